"""Reference of ba_match in numpy integers (tests/test_refmatch.py checks it, tests/test_gpu_match.py compares the GPU
against it exactly), and the named cases.

A separate formulation from the kernels': the Hamming distance by ``unpackbits``, the squared L2 distance by direct
int64 differences, the two nearest trains by a sort on the packed key ``distance << 32 | index``, the ratio tests in
f32 (HAMMING) and f64 on the squares (L2_U8) as include/ba.h states them, the cross-check by a column argmin. The
second formulation (``distances_alt``: a popcount table over the xor, norms minus twice the dot product in int64) is
what the kernels do and what test_refmatch.py holds the first one against.

Every distance is an integer, so every output has one right answer: nothing here has a tolerance."""
from functools import lru_cache

import numpy as np

# csrc/ba_match.h (test_match_abi.py compares): queries of a workgroup, trains of an LDS tile, rows / columns of an
# MFMA tile, descriptor bytes of one MFMA
QTILE, TTILE, MFMA, KSTEP = 64, 64, 16, 64
MAX_SLICES = 64
# include/ba.h
HAMMING, L2_U8 = 0, 1
MAX_BYTES = 256
COUNT_N = 7
KINDS = ("hamming", "l2_u8")
KIND_ID = {"hamming": HAMMING, "l2_u8": L2_U8}
# the descriptor size a case uses unless it names one: ORB's and byte SIFT's
DEFAULT_BYTES = {"hamming": 32, "l2_u8": 128}
# descriptor sizes the rectangular case runs at (include/ba.h: multiples of 4 in [4, 256]; 36 pads a k-step)
DESC_BYTES = {"hamming": (32, 64, 4, 256), "l2_u8": (128, 64, 36, 4, 256)}
# the sizes around every tile size T: 0, 1, 2, 3, T - 1, T, T + 1
EDGE_SIZES = sorted({0, 1, 2, 3} | {t + d for t in (MFMA, TTILE, QTILE) for d in (-1, 0, 1)})
# max_distance of the acceptance cases: between a lightly and a moderately disturbed copy (``noisy``)
MAX_DISTANCE = {"hamming": 30, "l2_u8": 100000}


# ---- the reference -------------------------------------------------------------------------------------------------

def distances(q, t, kind):
    """(n_q, n_t) int64: every query against every train."""
    q, t = np.asarray(q, dtype=np.uint8), np.asarray(t, dtype=np.uint8)
    out = np.zeros((len(q), len(t)), dtype=np.int64)
    if not len(q) or not len(t):
        return out
    if kind == "hamming":
        tb = np.unpackbits(t, axis=1)
        for i in range(len(q)):
            out[i] = (np.unpackbits(q[i])[None, :] != tb).sum(axis=1)
    else:
        t64 = t.astype(np.int64)
        for i in range(len(q)):
            diff = q[i].astype(np.int64)[None, :] - t64
            out[i] = (diff * diff).sum(axis=1)
    return out


_POP8 = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)


def distances_alt(q, t, kind):
    """The kernels' formulation: a popcount table over the xor; |a'|^2 + |b'|^2 - 2 a'.b' with a' = a - 128."""
    q, t = np.asarray(q, dtype=np.uint8), np.asarray(t, dtype=np.uint8)
    if not len(q) or not len(t):
        return np.zeros((len(q), len(t)), dtype=np.int64)
    if kind == "hamming":
        return _POP8[q[:, None, :] ^ t[None, :, :]].sum(axis=2)
    a = (q ^ 0x80).view(np.int8).astype(np.int64)
    b = (t ^ 0x80).view(np.int8).astype(np.int64)
    return (a * a).sum(axis=1)[:, None] + (b * b).sum(axis=1)[None, :] - 2 * (a @ b.T)


def top2(D):
    """The two smallest trains of every row under (distance, index): nn_idx, nn_dist (n_q, 2) int32, -1 = none."""
    nq, nt = D.shape
    idx = np.full((nq, 2), -1, dtype=np.int32)
    dist = np.full((nq, 2), -1, dtype=np.int32)
    if nt:
        key = np.sort((D.astype(np.uint64) << np.uint64(32)) | np.arange(nt, dtype=np.uint64)[None, :], axis=1)[:, :2]
        k = key.shape[1]
        idx[:, :k] = (key & np.uint64(0xFFFFFFFF)).astype(np.int32)
        dist[:, :k] = (key >> np.uint64(32)).astype(np.int32)
    return idx, dist


def match_pair(D, kind, ratio=0.7, max_distance=0, cross_check=False):
    """One pair from its distance matrix: nn_idx, nn_dist, and per query the count it falls into (2 accepted, 3 no
    second neighbour, 4 the ratio, 5 max_distance, 6 the cross-check: the first condition it fails)."""
    idx, dist = top2(D)
    nq = len(D)
    at = np.full(nq, 2, dtype=np.int32)
    r32 = np.float32(ratio if ratio > 0 else 0.7)
    for q in range(nq):
        d0, d1 = int(dist[q, 0]), int(dist[q, 1])
        if idx[q, 1] < 0:
            at[q] = 3
            continue
        if kind == "hamming":
            ok = bool(np.float32(d0) < r32 * np.float32(d1))  # one f32 product, one comparison
        else:
            ok = float(d0) < (float(r32) * float(r32)) * float(d1)
        if not ok:
            at[q] = 4
        elif max_distance > 0 and d0 > max_distance:
            at[q] = 5
        elif cross_check and int(np.argmin(D[:, idx[q, 0]])) != q:  # (argmin: the first, so the smallest query)
            at[q] = 6
    return idx, dist, at


def match(query, train, pair_range, kind, ratio=0.7, max_distance=0, cross_check=False, D=None):
    """Solver.match's dictionary, from the reference. ``D``: the pairs' distance matrices when the caller has them."""
    rng = np.asarray(pair_range, dtype=np.int64).reshape(-1, 4)
    P = len(rng)
    idx, dist, acc, mats, mbegin = [], [], [], [], [0]
    counts = np.zeros((P, COUNT_N), dtype=np.int32)
    for j, (qb, qe, tb, te) in enumerate(rng):
        Dj = distances(query[qb:qe], train[tb:te], kind) if D is None else D[j]
        i, d, at = match_pair(Dj, kind, ratio, max_distance, cross_check)
        idx.append(i); dist.append(d); acc.append((at == 2).astype(np.uint8))
        sel = np.nonzero(at == 2)[0]
        mats.append(np.stack([sel, i[sel, 0]], axis=1).astype(np.int32).reshape(-1, 2))
        mbegin.append(mbegin[-1] + len(sel))
        counts[j, 0], counts[j, 1] = qe - qb, te - tb
        for c in range(2, COUNT_N):
            counts[j, c] = int((at == c).sum())
    cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dtype=dt)  # noqa: E731
    return dict(nn_idx=cat(idx, (0, 2), np.int32), nn_dist=cat(dist, (0, 2), np.int32), accept=cat(acc, (0,), np.uint8),
                matches=cat(mats, (0, 2), np.int32), match_begin=np.array(mbegin, dtype=np.int32), pair_counts=counts,
                n_matches=mbegin[-1], n_pairs=P, n_rows=int((rng[:, 1] - rng[:, 0]).sum()),
                row_begin=np.concatenate([[0], np.cumsum(rng[:, 1] - rng[:, 0])]))


# ---- the inputs ----------------------------------------------------------------------------------------------------

def random_desc(rng, n, nbytes):
    return rng.integers(0, 256, size=(n, nbytes), dtype=np.uint8)


# how much a copy is disturbed: lightly (passes everything), moderately (passes the default ratio, fails MAX_DISTANCE),
# heavily (fails the default ratio): the share of flipped bits / the sigma of the added noise
LEVELS = {"hamming": (0.03, 0.2, 0.36), "l2_u8": (10.0, 50.0, 90.0)}


def noisy(rng, d, kind, level):
    d = np.asarray(d, dtype=np.uint8)
    if kind == "hamming":
        return d ^ np.packbits(rng.random(d.shape[:-1] + (8 * d.shape[-1],)) < level, axis=-1)
    return np.clip(d.astype(np.int64) + np.rint(rng.normal(0.0, level, d.shape)).astype(np.int64), 0, 255).astype(np.uint8)


def structured_pair(rng, nq, nt, nbytes, kind):
    """Random trains; query i is, by i % 5: a light copy of a train, a light copy of the SAME train as query i - 1 (one
    of the two fails the cross-check), a moderate copy, a heavy copy, a random descriptor."""
    t = random_desc(rng, nt, nbytes)
    q = random_desc(rng, nq, nbytes)
    if nt:
        src = 0
        for i in range(nq):
            mode = i % 5
            if mode != 1:
                src = (7 * i + 3) % nt
            if mode < 4:
                q[i] = noisy(rng, t[src], kind, LEVELS[kind][{0: 0, 1: 0, 2: 1, 3: 2}[mode]])
    return q, t


def batch(kind, nbytes, shapes, seed):
    """One descriptor set per pair, concatenated: query, train, pair_range."""
    rng = np.random.default_rng(seed)
    qs, ts, pr, q0, t0 = [], [], [], 0, 0
    for nq, nt in shapes:
        q, t = structured_pair(rng, nq, nt, nbytes, kind)
        qs.append(q); ts.append(t)
        pr.append((q0, q0 + nq, t0, t0 + nt))
        q0 += nq; t0 += nt
    return (np.concatenate(qs).reshape(-1, nbytes), np.concatenate(ts).reshape(-1, nbytes),
            np.array(pr, dtype=np.int32).reshape(-1, 4))


def _case_shapes_q(kind, nbytes):
    return batch(kind, nbytes, [(n, 33) for n in EDGE_SIZES], 11) + ({},)


def _case_shapes_t(kind, nbytes):
    return batch(kind, nbytes, [(17, n) for n in EDGE_SIZES], 12) + ({},)


def _case_shapes_square(kind, nbytes):
    return batch(kind, nbytes, [(n, n) for n in EDGE_SIZES], 13) + ({},)


def _case_rect(kind, nbytes):
    rng = np.random.default_rng(14 + nbytes)
    return random_desc(rng, 17, nbytes), random_desc(rng, 33, nbytes), np.array([[0, 17, 0, 33]], dtype=np.int32), {}


def _case_ties_train(kind, nbytes):
    """Duplicated trains: the smaller index is first, and the ratio fails at d0 = d1 even at ratio 1."""
    rng = np.random.default_rng(15)
    t = random_desc(rng, 40, nbytes)
    t[[9, 21, 38]] = t[4]
    t[30] = t[17]
    t[2] = t[35]
    q = noisy(rng, t[[4, 17, 35, 0, 9, 38, 12]], kind, LEVELS[kind][0])
    q[3] = t[0]
    q = np.concatenate([q, random_desc(rng, 4, nbytes)])
    return q, t, np.array([[0, len(q), 0, 40]], dtype=np.int32), dict(ratio=1.0)


def _case_ties_query(kind, nbytes):
    """Duplicated queries under cross_check: the smaller query index wins its train."""
    q, t, pr = batch(kind, nbytes, [(30, 25)], 16)
    q[[6, 11, 20]] = q[5]
    q[26] = q[0]
    return q, t, pr, dict(cross_check=True)


def _case_extreme(kind, nbytes=MAX_BYTES):
    """All-0 against all-255 at the longest descriptor (8 desc_bytes, desc_bytes 255^2: the int32 range and the shift
    by 128), and identical descriptors (d0 = 0)."""
    q = np.zeros((6, MAX_BYTES), dtype=np.uint8)
    t = np.zeros((5, MAX_BYTES), dtype=np.uint8)
    q[1] = 255; q[3] = 255; q[4, ::2] = 255; q[5] = 128
    t[0] = 255; t[2] = 255; t[3, ::2] = 255; t[4] = 127
    pr = np.array([[0, 6, 0, 5], [0, 2, 0, 1], [1, 4, 1, 2]], dtype=np.int32)
    return q, t, pr, dict(ratio=1.0)


def _case_slices(kind, nbytes):
    """One pair with more train tiles than one: the host slices it (MIBA_MATCH_SLICES unset)."""
    return batch(kind, nbytes, [(QTILE + 6, 5 * TTILE + 7)], 17) + ({},)


def _case_batch1(kind, nbytes):
    return batch(kind, nbytes, [(50, 70)], 18) + ({},)


def _case_batch2(kind, nbytes):
    return batch(kind, nbytes, [(20, 0), (33, 65)], 19) + ({},)


def _case_batch9(kind, nbytes):
    """Nine pairs over shared sets: empty pairs, overlapping ranges, one train."""
    q, t, _ = batch(kind, nbytes, [(90, 130)], 20)
    pr = np.array([[0, 40, 0, 60], [10, 80, 30, 130], [5, 5, 0, 130], [0, 90, 50, 50], [0, 90, 0, 130], [60, 90, 129, 130],
                   [89, 90, 0, 2], [0, 0, 0, 0], [20, 85, 64, 128]], dtype=np.int32)
    return q, t, pr, {}


def _case_one_vs_five(kind, nbytes):
    """One query set against five train sets: one copy of the queries."""
    rng = np.random.default_rng(21)
    q, t, _ = batch(kind, nbytes, [(45, 40)], 21)
    ts = [t] + [noisy(rng, t[rng.permutation(40)[: 40 - 3 * k]], kind, LEVELS[kind][0]) for k in range(1, 5)]
    begin = np.concatenate([[0], np.cumsum([len(x) for x in ts])])
    pr = np.array([[0, 45, begin[k], begin[k + 1]] for k in range(5)], dtype=np.int32)
    return q, np.concatenate(ts), pr, {}


def _case_accept(kind, nbytes):
    """Every count of the chain: structured pairs, a pair with one train and a pair with none."""
    return batch(kind, nbytes, [(60, 45), (7, 1), (4, 0), (35, 80)], 22) + ({},)


# name -> builder(kind, desc_bytes) -> query, train, pair_range, kwargs of Solver.match
CASES = {
    "shapes-q": _case_shapes_q, "shapes-t": _case_shapes_t, "shapes-square": _case_shapes_square,
    "rect-17x33": _case_rect, "ties-train": _case_ties_train, "ties-query": _case_ties_query, "extreme": _case_extreme,
    "slices": _case_slices, "batch-1": _case_batch1, "batch-2": _case_batch2, "batch-9": _case_batch9,
    "one-vs-five": _case_one_vs_five, "accept": _case_accept,
}
# the acceptance settings the "accept" case runs at (ratio, max_distance on, cross_check)
ACCEPT_SETTINGS = [(r, m, c) for r in (0.7, 1.0, 0.5) for m in (False, True) for c in (False, True)]


@lru_cache(maxsize=None)
def case_inputs(name, kind, nbytes=None):
    q, t, pr, kw = CASES[name](kind, nbytes or DEFAULT_BYTES[kind])
    for a in (q, t, pr):
        a.setflags(write=False)
    return q, t, pr, kw


@lru_cache(maxsize=None)
def case_distances(name, kind, nbytes=None):
    q, t, pr, _ = case_inputs(name, kind, nbytes)
    return tuple(distances(q[a:b], t[c:d], kind) for a, b, c, d in pr)


@lru_cache(maxsize=None)
def case_reference(name, kind, nbytes=None, **over):
    """The reference's dictionary of a case at its own settings, ``over`` replacing them."""
    q, t, pr, kw = case_inputs(name, kind, nbytes)
    return match(q, t, pr, kind, D=case_distances(name, kind, nbytes), **{**kw, **over})


# ---- the end-to-end inputs -----------------------------------------------------------------------------------------

def two_keyframes(seed, n_feat=500, n_shared=350, nbytes=32, flip=0.06):
    """Two keyframes of n_feat features, n_shared landmarks in common at shuffled positions, every observation a copy
    of its landmark's descriptor with ``flip`` of the bits flipped. Returns desc_a, desc_b, ids_a, ids_b."""
    rng = np.random.default_rng(seed)
    n_ids = 2 * n_feat - n_shared
    desc = random_desc(rng, n_ids, nbytes)
    ids_a = rng.permutation(np.arange(n_feat))
    ids_b = rng.permutation(np.concatenate([np.arange(n_shared), np.arange(n_feat, n_ids)]))
    return (noisy(rng, desc[ids_a], "hamming", flip), noisy(rng, desc[ids_b], "hamming", flip),
            ids_a.astype(np.int64), ids_b.astype(np.int64))
