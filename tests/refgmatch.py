"""Reference of ba_guided_match (tests/test_refgmatch.py checks it, tests/test_gpu_gmatch.py compares the GPU against
it exactly), and the named cases.

The projection and the two gates (the pixel disc, the relative depth) are evaluated in ``np.longdouble``; everything
else is integer work: the distances are tests/refmatch.py's, the two nearest keypoints of a window a sort on the key
``distance << 32 | keypoint index``, the one-to-one pick a minimum over ``(d0, row)``. ``guided`` looks at every
keypoint of the frame's range (no grid); ``guided_grid`` is the second statement, which bins the keypoints into cells
and visits the cell rectangle of a window as the kernels do.

Every floating-point decision is returned with its margin (``margin``: the smallest relative distance of a compared
value from its threshold over the whole case), so a test can require that no decision is within 1e-6 of flipping: the
float64 kernels then take the same decisions as the longdouble reference and every integer output has one right
answer."""
from functools import lru_cache

import numpy as np

import refmatch as rm

LD = np.longdouble
COUNT_N = 9  # include/ba.h BA_GMATCH_COUNT_N
ACCEPTED, BEHIND, OUTSIDE, EMPTY, RATIO, MAX_DISTANCE, ONE_TO_ONE = range(7)
MIN_CELL = 8  # csrc/ba_gmatch_host.h GMATCH_MIN_CELL
MIN_MARGIN = 1e-6
INT_ARRAYS = ("nn_kp", "nn_dist", "status", "n_in_window", "matches", "match_begin", "frame_counts")
# descriptor sizes the small case runs at
DESC_BYTES = {"hamming": (32, 4, 64, 256), "l2_u8": (128, 36, 4, 256)}
CAND_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)
CELLS = (8, 16, 64, 4096)
MAX_DISTANCE_AT = {"hamming": 30, "l2_u8": 100000}


def default_cell(radius):
    c = MIN_CELL
    while c < radius:
        c *= 2
    return c


# ---- the reference -------------------------------------------------------------------------------------------------

def project(X, pose, intr):
    """u, v, z (longdouble) of the world points X (n, 3) in the camera T_w_c = pose (qx qy qz qw tx ty tz)."""
    q = np.asarray(pose, dtype=LD)
    qx, qy, qz, qw = q[:4]
    d = np.asarray(X, dtype=LD).reshape(-1, 3) - q[4:7]
    one, two = LD(1), LD(2)
    r00 = one - two * (qy * qy + qz * qz); r10 = two * (qx * qy + qw * qz); r20 = two * (qx * qz - qw * qy)
    r01 = two * (qx * qy - qw * qz); r11 = one - two * (qx * qx + qz * qz); r21 = two * (qy * qz + qw * qx)
    r02 = two * (qx * qz + qw * qy); r12 = two * (qy * qz - qw * qx); r22 = one - two * (qx * qx + qy * qy)
    x = r00 * d[:, 0] + r10 * d[:, 1] + r20 * d[:, 2]
    y = r01 * d[:, 0] + r11 * d[:, 1] + r21 * d[:, 2]
    z = r02 * d[:, 0] + r12 * d[:, 1] + r22 * d[:, 2]
    fx, fy, cx, cy = (LD(v) for v in intr)
    with np.errstate(all="ignore"):
        return fx * x / z + cx, fy * y / z + cy, z


def _normalise(points, kp_uv, frame_pose, frame_range, cand):
    poses = np.asarray(frame_pose, dtype=np.float64).reshape(-1, 7)
    F = len(poses)
    rng = np.tile([[0, len(kp_uv)]], (F, 1)) if frame_range is None else np.asarray(frame_range, dtype=np.int64).reshape(-1, 2)
    if cand is None:
        cand = [np.arange(len(points))] * F
    return poses, rng, [np.asarray(c, dtype=np.int64).reshape(-1) for c in cand]


def _frame_gates(points, kp_uv, kp_depth, pose, intr, width, height, rb, re, c, radius, min_depth, depth_tol):
    """One frame entry: u, v, z, the row status 0 / 1 / 2, the window mask (n_cand, n_kp) and the smallest margin."""
    md = LD(min_depth if min_depth > 0 else 1e-15)
    u, v, z = project(points[c], pose, intr)
    behind = ~(z > md)
    with np.errstate(all="ignore"):
        inside = (u >= 0) & (u < width) & (v >= 0) & (v < height)
    st = np.where(behind, BEHIND, np.where(inside, ACCEPTED, OUTSIDE))
    margin = [np.inf]
    if len(c):
        margin.append(float((np.abs(z - md) / np.maximum(np.abs(z), md)).min()))
    live = ~behind
    if live.any():
        W, H = LD(width), LD(height)
        margin.append(float(np.minimum(np.minimum(np.abs(u[live]), np.abs(u[live] - W)) / W,
                                       np.minimum(np.abs(v[live]), np.abs(v[live] - H)) / H).min()))
    kuv = np.asarray(kp_uv[rb:re], dtype=LD).reshape(-1, 2)
    r2 = LD(radius) * LD(radius)
    ok = st == ACCEPTED
    with np.errstate(all="ignore"):
        du = kuv[None, :, 0] - np.where(ok, u, 0)[:, None]
        dv = kuv[None, :, 1] - np.where(ok, v, 0)[:, None]
        s = du * du + dv * dv
        win = (s <= r2) & ok[:, None]
        if ok.any() and kuv.shape[0]:
            margin.append(float((np.abs(s[ok] - r2) / r2).min()))
        if kp_depth is not None and depth_tol > 0 and win.any():
            dk = np.asarray(kp_depth[rb:re], dtype=LD)
            gated = win & (dk > 1e-15)[None, :]
            lim = LD(depth_tol) * z[:, None]
            dev = np.abs(dk[None, :] - z[:, None])
            if gated.any():
                margin.append(float((np.abs(dev - lim) / lim)[gated].min()))
            win &= ~(gated & ~(dev <= lim))
    u = np.where(behind, 0, u)
    v = np.where(behind, 0, v)
    return u, v, z, st, win, min(margin)


def _chain(d0, d1, has1, kind, r32, max_distance):
    if has1:
        if kind == "hamming":
            ok = bool(np.float32(d0) < r32 * np.float32(d1))
        else:
            ok = float(d0) < (float(r32) * float(r32)) * float(d1)
        if not ok:
            return RATIO
    if max_distance > 0 and d0 > max_distance:
        return MAX_DISTANCE
    return ACCEPTED


def _finish(rows, poses, rng, cand, one_to_one, margin):
    """rows[f]: (nn_kp, nn_dist, status before the one-to-one pick, n_in_window, proj) of frame entry f."""
    F = len(poses)
    counts = np.zeros((F, COUNT_N), dtype=np.int32)
    nn_kp, nn_dist, status, n_win, proj, mats, mbegin = [], [], [], [], [], [], [0]
    for f in range(F):
        kp, dist, st, nw, pr = rows[f]
        st = st.copy()
        if one_to_one:
            best = {}
            for r in np.nonzero(st == ACCEPTED)[0]:
                key = (int(dist[r, 0]), int(r))
                if kp[r, 0] not in best or key < best[kp[r, 0]]:
                    best[kp[r, 0]] = key
            for r in np.nonzero(st == ACCEPTED)[0]:
                if best[kp[r, 0]][1] != r:
                    st[r] = ONE_TO_ONE
        sel = np.nonzero(st == ACCEPTED)[0]
        mats.append(np.stack([cand[f][sel], kp[sel, 0]], axis=1).astype(np.int32).reshape(-1, 2))
        mbegin.append(mbegin[-1] + len(sel))
        counts[f, 0], counts[f, 1] = len(cand[f]), rng[f, 1] - rng[f, 0]
        for s in range(7):
            counts[f, 2 + s] = int((st == s).sum())
        nn_kp.append(kp); nn_dist.append(dist); status.append(st.astype(np.uint8)); n_win.append(nw); proj.append(pr)
    cat = lambda parts, shape, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dtype=dt)  # noqa: E731
    cand_begin = np.concatenate([[0], np.cumsum([len(c) for c in cand])]).astype(np.int32)
    return dict(nn_kp=cat(nn_kp, (0, 2), np.int32), nn_dist=cat(nn_dist, (0, 2), np.int32), status=cat(status, (0,), np.uint8),
                n_in_window=cat(n_win, (0,), np.int32), proj=cat(proj, (0, 3), LD), matches=cat(mats, (0, 2), np.int32),
                match_begin=np.array(mbegin, dtype=np.int32), frame_counts=counts, n_matches=mbegin[-1], n_frames=F,
                n_rows=int(cand_begin[-1]), cand_begin=cand_begin,
                cand_pt=cat([c for c in cand], (0,), np.int32), margin=margin)


def guided(points, pt_desc, kp_uv, kp_desc, frame_pose, intr, width, height, frame_range=None, cand=None, kp_depth=None,
           kind="hamming", radius=15.0, ratio=0.7, max_distance=0, min_depth=0.0, depth_tol=0.0, one_to_one=True, cell_px=0):
    """Solver.guided_match's dictionary from the reference, with ``margin``. Every keypoint of the range is looked at:
    ``cell_px`` has no part in it."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    kp_uv = np.asarray(kp_uv, dtype=np.float64).reshape(-1, 2)
    poses, rng, cand = _normalise(points, kp_uv, frame_pose, frame_range, cand)
    r32 = np.float32(ratio if ratio > 0 else 0.7)
    rows, margin = [], np.inf
    none = np.int64(1) << 62
    for f in range(len(poses)):
        rb, re = rng[f]
        c = cand[f]
        u, v, z, st, win, m = _frame_gates(points, kp_uv, kp_depth, poses[f], intr, width, height, rb, re, c, radius,
                                           min_depth, depth_tol)
        margin = min(margin, m)
        n = len(c)
        kp = np.full((n, 2), -1, dtype=np.int32)
        dist = np.full((n, 2), -1, dtype=np.int32)
        if n and re > rb:
            D = rm.distances(pt_desc[c], kp_desc[rb:re], kind)
            key = np.where(win, (D << 32) | np.arange(re - rb, dtype=np.int64)[None, :], none)
            key = np.sort(key, axis=1)[:, :2]
            for j in range(key.shape[1]):
                has = key[:, j] != none
                kp[has, j] = (key[has, j] & 0xFFFFFFFF).astype(np.int32)
                dist[has, j] = (key[has, j] >> 32).astype(np.int32)
        st = st.copy()
        for r in range(n):
            if st[r] == ACCEPTED:
                st[r] = EMPTY if kp[r, 0] < 0 else _chain(int(dist[r, 0]), int(dist[r, 1]), kp[r, 1] >= 0, kind, r32, max_distance)
        rows.append((kp, dist, st, win.sum(axis=1).astype(np.int32), np.stack([u, v, z], axis=1)))
    return _finish(rows, poses, rng, cand, one_to_one, margin)


def guided_grid(points, pt_desc, kp_uv, kp_desc, frame_pose, intr, width, height, frame_range=None, cand=None, kp_depth=None,
                kind="hamming", radius=15.0, ratio=0.7, max_distance=0, min_depth=0.0, depth_tol=0.0, one_to_one=True, cell_px=0):
    """The second statement: the keypoints binned into cells of ``cell_px`` (clamped into the border cells), a window's
    cell rectangle widened by a pixel, the gates and the distances per visited keypoint, a running best two."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    kp_uv = np.asarray(kp_uv, dtype=np.float64).reshape(-1, 2)
    poses, rng, cand = _normalise(points, kp_uv, frame_pose, frame_range, cand)
    cell = cell_px if cell_px > 0 else default_cell(radius)
    gw, gh = -(-width // cell), -(-height // cell)
    r32 = np.float32(ratio if ratio > 0 else 0.7)
    md = LD(min_depth if min_depth > 0 else 1e-15)
    r2 = LD(radius) * LD(radius)
    clamp = lambda x, n: 0 if not x > 0 else int(min(np.floor(x / cell), n - 1))  # noqa: E731
    rows, margin = [], np.inf
    for f in range(len(poses)):
        rb, re = (int(x) for x in rng[f])
        c = cand[f]
        bins = {}
        for k in range(rb, re):
            bins.setdefault((clamp(kp_uv[k, 0], gw), clamp(kp_uv[k, 1], gh)), []).append(k)
        u, v, z = project(points[c], poses[f], intr)
        n = len(c)
        kp = np.full((n, 2), -1, dtype=np.int32)
        dist = np.full((n, 2), -1, dtype=np.int32)
        st = np.zeros(n, dtype=np.int64)
        nw = np.zeros(n, dtype=np.int32)
        pr = np.zeros((n, 3), dtype=LD)
        for r in range(n):
            pr[r] = (u[r], v[r], z[r])
            if not z[r] > md:
                st[r] = BEHIND
                pr[r, :2] = 0
                continue
            if not (0 <= u[r] < width and 0 <= v[r] < height):
                st[r] = OUTSIDE
                continue
            best = []
            for cy in range(clamp(float(v[r]) - radius - 1, gh), clamp(float(v[r]) + radius + 1, gh) + 1):
                for cx in range(clamp(float(u[r]) - radius - 1, gw), clamp(float(u[r]) + radius + 1, gw) + 1):
                    for k in bins.get((cx, cy), ()):
                        du, dv = LD(kp_uv[k, 0]) - u[r], LD(kp_uv[k, 1]) - v[r]
                        if not du * du + dv * dv <= r2:
                            continue
                        if kp_depth is not None and depth_tol > 0 and kp_depth[k] > 1e-15 and \
                                not abs(LD(kp_depth[k]) - z[r]) <= LD(depth_tol) * z[r]:
                            continue
                        nw[r] += 1
                        d = int(rm.distances_alt(pt_desc[c[r]][None], kp_desc[k][None], kind)[0, 0])
                        best = sorted(best + [(d, k - rb)])[:2]
            for j, (d, k) in enumerate(best):
                kp[r, j], dist[r, j] = k, d
            st[r] = EMPTY if not best else _chain(best[0][0], best[1][0] if len(best) > 1 else -1, len(best) > 1, kind, r32,
                                                  max_distance)
        rows.append((kp, dist, st, nw, pr))
    return _finish(rows, poses, rng, cand, one_to_one, margin)


# ---- the inputs ----------------------------------------------------------------------------------------------------

def pose_of(angle, t, axis=(0.0, 1.0, 0.0)):
    """T_w_c as [qx, qy, qz, qw, t]."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    return np.array([*(np.sin(angle / 2) * a), np.cos(angle / 2), *t])


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def backproject(uv, z, pose, intr):
    """The world points that project to the pixels uv at depth z in the camera ``pose``."""
    fx, fy, cx, cy = intr
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), (len(uv),))
    pc = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], axis=1)
    return pc @ _rot(pose[:4]).T + pose[4:]


W0, H0 = 100, 75  # the cases' image: no multiple of any cell size
K0 = np.array([90.0, 88.0, 49.63, 37.29])
POSE0 = pose_of(0.07, [0.05, -0.02, 0.01], axis=(0.3, 1.0, -0.2))


def scene(kind, nbytes, seed, n_lm, n_extra, radius=15.0, width=W0, height=H0, pose=POSE0, intr=K0):
    """A frame's landmarks and keypoints. Landmarks: pixels drawn over the image and a margin around it, depths in
    [2, 6], every 11th behind the camera. Keypoints: for 3 landmarks of 4 an observation within 1.2 radii of the
    projection (so some leave the window), by turns a light / light / moderate / heavy copy of the descriptor with a
    depth that is right, missing, or 30 % off; for every 5th a second light copy nearby (the ratio test's failure);
    then n_extra keypoints of random descriptors over the image and 10 px around it. Shuffled."""
    rng = np.random.default_rng(seed)
    px = np.stack([rng.uniform(-0.06 * width, 1.06 * width, n_lm), rng.uniform(-0.06 * height, 1.06 * height, n_lm)], axis=1)
    z = rng.uniform(2.0, 6.0, n_lm)
    z[5::11] *= -1
    X = backproject(px, z, pose, intr)
    desc = rm.random_desc(rng, n_lm, nbytes)
    kuv, kd, kz = [], [], []
    for i in range(n_lm):
        if i % 4 == 3 or z[i] < 0:
            continue
        rho, phi = 1.2 * radius * np.sqrt(rng.uniform()), rng.uniform(0, 2 * np.pi)
        kuv.append(px[i] + rho * np.array([np.cos(phi), np.sin(phi)]))
        kd.append(rm.noisy(rng, desc[i], kind, rm.LEVELS[kind][(0, 0, 1, 2)[i % 4 if i % 8 else 3]]))
        kz.append((z[i], 0.0, 1.3 * z[i])[(i // 3) % 3 if i % 2 else 0])
        if i % 5 == 0:
            kuv.append(kuv[-1] + rng.uniform(-2, 2, 2))
            kd.append(rm.noisy(rng, desc[i], kind, rm.LEVELS[kind][0]))
            kz.append(z[i])
    kuv += list(np.stack([rng.uniform(-10, width + 10, n_extra), rng.uniform(-10, height + 10, n_extra)], axis=1))
    kd += list(rm.random_desc(rng, n_extra, nbytes))
    kz += list(rng.uniform(2.0, 6.0, n_extra))
    order = rng.permutation(len(kuv))
    return dict(points=X, pt_desc=desc, kp_uv=np.array(kuv).reshape(-1, 2)[order], kp_desc=np.array(kd, dtype=np.uint8).reshape(-1, nbytes)[order],
                kp_depth=np.array(kz)[order], frame_pose=pose[None].copy(), intr=intr, width=width, height=height)


def _case_small(kind, nbytes):
    return scene(kind, nbytes, 41 + nbytes, 40, 30), {}


def _case_cand_counts(kind, nbytes):
    """One entry per candidate count around the search kernel's wave and the scanning workgroup, over two keypoint
    ranges (entries alternate between them) and poses that differ a little."""
    a = scene(kind, nbytes, 42, 257, 60)
    b = scene(kind, nbytes, 43, 257, 40)
    rng = np.random.default_rng(44)
    na = len(a["kp_uv"])
    args = dict(a, kp_uv=np.concatenate([a["kp_uv"], b["kp_uv"]]), kp_desc=np.concatenate([a["kp_desc"], b["kp_desc"]]),
                kp_depth=np.concatenate([a["kp_depth"], b["kp_depth"]]))
    n = len(CAND_COUNTS)
    args["frame_pose"] = np.stack([pose_of(0.07 + 0.002 * f, [0.05 + 0.01 * f, -0.02, 0.01], axis=(0.3, 1.0, -0.2)) for f in range(n)])
    args["frame_range"] = np.array([[0, na] if f % 2 == 0 else [na, len(args["kp_uv"])] for f in range(n)], dtype=np.int32)
    args["cand"] = [rng.permutation(257)[:c] for c in CAND_COUNTS]
    return args, {}


def _case_empty(kind, nbytes):
    """Entries without keypoints, entries without candidates, both, and a plain one between them."""
    args = scene(kind, nbytes, 45, 30, 20)
    nk = len(args["kp_uv"])
    args["frame_pose"] = np.repeat(args["frame_pose"], 5, axis=0)
    args["frame_range"] = np.array([[0, 0], [0, nk], [7, 7], [0, nk], [nk, nk]], dtype=np.int32)
    args["cand"] = [np.arange(30), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.arange(30)[::-1], np.arange(3)]
    return args, {}


IDENT = pose_of(0.0, [0.0, 0.0, 0.0])
K_INT = np.array([64.0, 64.0, 48.0, 32.0])  # with depth 2 and x, y multiples of 1 / 32 the pixels are exact


def _sculpted(kind, nbytes, seed, lm_px, kp_px, copies=None):
    """Landmarks at the pixels lm_px (identity pose, depth 2: exact pixels) and keypoints at kp_px; keypoint j copies
    the descriptor of landmark copies[j] lightly (None / -1: a random descriptor)."""
    rng = np.random.default_rng(seed)
    lm_px, kp_px = np.asarray(lm_px, dtype=np.float64).reshape(-1, 2), np.asarray(kp_px, dtype=np.float64).reshape(-1, 2)
    X = np.stack([(lm_px[:, 0] - K_INT[2]) / 32.0, (lm_px[:, 1] - K_INT[3]) / 32.0, np.full(len(lm_px), 2.0)], axis=1)
    desc = rm.random_desc(rng, len(lm_px), nbytes)
    kd = rm.random_desc(rng, len(kp_px), nbytes)
    for j, i in enumerate(copies if copies is not None else []):
        if i >= 0:
            kd[j] = rm.noisy(rng, desc[i], kind, rm.LEVELS[kind][0])
    return dict(points=X, pt_desc=desc, kp_uv=kp_px, kp_desc=kd, kp_depth=np.full(len(kp_px), 2.0), frame_pose=IDENT[None].copy(),
                intr=K_INT, width=W0, height=H0)


def _case_boundaries(kind, nbytes):
    """Projections on cell boundaries of every cell size (multiples of 8, 16 and 64) and
    keypoints exactly on them and a quarter pixel to either side; the radius is below one cell."""
    lm = [(x, y) for x in (8.0, 16.0, 64.0, 96.0) for y in (8.0, 16.0, 64.0, 72.0)]
    kp, copies = [], []
    for x in (0.0, 8.0, 16.0, 64.0, 96.0):
        for y in (8.0, 16.0, 64.0):
            kp += [(x, y), (x - 0.25, y), (x + 0.25, y - 0.25), (x, y + 2.5)]
            copies += [lm.index((x, y)) if (x, y) in lm else -1, -1, -1, -1]
    return _sculpted(kind, nbytes, 46, lm, kp, copies), dict(radius=3.0)


def _case_wide(kind, nbytes):
    """A radius of several cells at the smallest cell: the window's rectangle is 11 x 11 cells and is clipped."""
    return scene(kind, nbytes, 47, 40, 50, radius=40.0), dict(radius=40.0, cell_px=8)


def _case_borders(kind, nbytes):
    """Windows clipped at the four borders and the four corners, with keypoints outside the image inside them (they
    sit in the border cells) and far outside it."""
    lm = [(2.0, 36.0), (98.0, 36.0), (50.0, 1.5), (50.0, 73.5), (1.0, 1.0), (99.0, 1.0), (1.0, 74.0), (99.0, 74.0), (50.0, 36.0)]
    kp, copies = [], []
    for i, (x, y) in enumerate(lm):
        sx, sy = (-1 if x < 50 else 1), (-1 if y < 36 else 1)
        kp += [(x + 6.0 * sx, y + 5.0 * sy), (x - 3.0 * sx, y - 2.0 * sy), (x + 200.0 * sx, y), (x, y + 200.0 * sy)]
        copies += [i, -1, i, -1]
    return _sculpted(kind, nbytes, 48, lm, kp, copies), dict(radius=15.0)


def _case_crowd(kind, nbytes):
    """300 keypoints on one pixel (one cell holds them all, whatever its size) with distinct descriptors, two of them
    equal to each other and nearest to landmark 0: the smaller index is first."""
    lm = [(41.0, 21.0), (44.0, 19.0), (80.0, 60.0)]
    kp = [(40.25, 20.5)] * 300 + [(81.0, 61.0), (10.0, 10.0)]
    copies = [-1] * 302
    copies[117] = copies[250] = 0
    copies[33] = 1
    copies[300] = 2
    args = _sculpted(kind, nbytes, 49, lm, kp, copies)
    args["kp_desc"][250] = args["kp_desc"][117]
    return args, dict(radius=6.0, ratio=1.0)


def _case_ties(kind, nbytes):
    """Equal descriptors in one window (the smaller keypoint index is first, and the ratio fails at d0 = d1 even at
    ratio 1), and one-to-one ties: landmarks 3, 4, 5 share a descriptor and a pixel, so they choose the same keypoint
    at the same distance and the smallest row keeps it; landmark 6 reaches it at a larger distance."""
    lm = [(20.0, 20.0), (60.0, 20.0), (20.0, 56.0), (60.0, 56.0), (60.0, 56.0), (60.0, 56.0), (61.0, 55.0), (90.0, 40.0)]
    kp = [(21.0, 21.0), (19.0, 22.0), (22.0, 18.0), (61.0, 21.0), (21.0, 55.0), (59.0, 57.0), (90.5, 40.5), (63.0, 20.0)]
    copies = [0, 0, -1, 1, 2, 3, 7, 1]
    args = _sculpted(kind, nbytes, 50, lm, kp, copies)
    args["kp_desc"][1] = args["kp_desc"][0]
    args["kp_desc"][7] = args["kp_desc"][3]
    args["pt_desc"][4] = args["pt_desc"][5] = args["pt_desc"][3]
    rng = np.random.default_rng(51)
    args["pt_desc"][6] = rm.noisy(rng, args["pt_desc"][3], kind, rm.LEVELS[kind][1])
    args["cand"] = [np.array([7, 5, 3, 4, 6, 0, 1, 2])]
    return args, dict(radius=8.0, ratio=1.0)


def _case_accept(kind, nbytes):
    """Every status of the chain: the general scene with its behind / outside landmarks, light to heavy copies,
    second copies nearby, missing and wrong depths, and two landmarks with one descriptor."""
    args = scene(kind, nbytes, 52, 120, 60)
    args["pt_desc"][[11, 19, 31, 43]] = args["pt_desc"][[9, 17, 29, 41]]
    args["points"][[11, 19, 31, 43]] = args["points"][[9, 17, 29, 41]] + 1e-3
    return args, {}


def _case_hypotheses(kind, nbytes):
    """Five pose hypotheses over one shared keypoint range."""
    args = scene(kind, nbytes, 53, 80, 40)
    args["frame_pose"] = np.stack([pose_of(0.07 + 0.004 * f, [0.05 - 0.02 * f, -0.02 + 0.01 * f, 0.01], axis=(0.3, 1.0, -0.2))
                                   for f in range(5)])
    return args, {}


def _case_all_in_view(kind, nbytes):
    """Every landmark in front of the camera and inside the image, a radius above the image diagonal and no depth
    gate: the window is the whole range, so the neighbours are Solver.match's."""
    args = scene(kind, nbytes, 54, 60, 40)
    rng = np.random.default_rng(55)
    px = np.stack([rng.uniform(1, W0 - 1, 60), rng.uniform(1, H0 - 1, 60)], axis=1)
    args["points"] = backproject(px, rng.uniform(2.0, 6.0, 60), POSE0, K0)
    return args, dict(radius=400.0, one_to_one=False)


CASES = {
    "small": _case_small, "cand-counts": _case_cand_counts, "empty": _case_empty, "boundaries": _case_boundaries,
    "wide": _case_wide, "borders": _case_borders, "crowd": _case_crowd, "ties": _case_ties, "accept": _case_accept,
    "hypotheses": _case_hypotheses, "all-in-view": _case_all_in_view,
}
# the settings the "accept" case runs at: ratio, max_distance on, depth_tol, one_to_one
ACCEPT_SETTINGS = [(r, m, t, o) for r in (0.7, 1.0) for m in (False, True) for t in (0.0, 0.1) for o in (False, True)]


@lru_cache(maxsize=None)
def case_inputs(name, kind, nbytes=None):
    args, kw = CASES[name](kind, nbytes or rm.DEFAULT_BYTES[kind])
    for a in args.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return args, kw


def accept_kw(kind, ratio, md, tol, one):
    return dict(ratio=ratio, max_distance=MAX_DISTANCE_AT[kind] if md else 0, depth_tol=tol, one_to_one=one)


_REF = {}


def case_reference(name, kind, nbytes=None, **over):
    """The reference's dictionary of a case at its own settings, ``over`` replacing them (computed once, shared)."""
    key = (name, kind, nbytes, tuple(sorted(over.items())))
    if key not in _REF:
        args, kw = case_inputs(name, kind, nbytes)
        _REF[key] = guided(**args, kind=kind, **{**kw, **over})
    return _REF[key]


# ---- the pipeline fixtures -----------------------------------------------------------------------------------------

def cpu_guided(points, pt_desc, kp_uv, kp_desc, frame_pose, intr, width, height, matches=True, counts=False, proj=False, **kw):
    """The reference under Solver.guided_match's signature: what miba.window / miba.matching take as ``guided_match``."""
    return guided(points, pt_desc, kp_uv, kp_desc, frame_pose, intr, width, height, **kw)


HIDDEN = dict(n_keyframes=6, n_landmarks=400, seed=2, k=5, desc_seed=7, flip=0.06)


def hidden_links():
    """A synthetic sequence with descriptors in which keyframe k lost every link to a landmark an earlier keyframe
    also observes: (keyframes, landmarks, intr, k, deleted) with deleted the {local id: landmark id} taken out."""
    from miba import matching, sequence
    kfs, lms, K0, _ = sequence.make_tum_sequence(n_keyframes=HIDDEN["n_keyframes"], n_landmarks=HIDDEN["n_landmarks"],
                                                 seed=HIDDEN["seed"])
    matching.attach_descriptors(kfs, seed=HIDDEN["desc_seed"], kind="hamming", flip=HIDDEN["flip"])
    k = HIDDEN["k"]
    earlier = set()
    for kf in kfs[:k]:
        earlier.update(kf.global_points_map.values())
    deleted = {i: g for i, g in kfs[k].global_points_map.items() if g in earlier}
    kfs[k].global_points_map = {i: g for i, g in kfs[k].global_points_map.items() if g not in earlier}
    return kfs, lms, K0, k, deleted


SWEEPS = dict(n=3, n_lm=260, per_kf=180)
K_SWEEP = np.array([525.0, 525.0, 319.5, 239.5])


def two_sweeps():
    """Two sweeps of three keyframes past one scene; the second sweep's landmarks carry new ids (id + n_lm) and its own
    copy of the points: the map after a loop closure that has not fused its duplicates (the construction of
    test_gpu_match.py::test_matched_edges_between_keyframes_without_a_shared_id, with the pixels filled in).
    Returns keyframes, landmarks {id: point}, intr, the loop pairs."""
    from miba import matching, posegraph, window
    rng = np.random.default_rng(8)
    n, n_lm, per_kf = SWEEPS["n"], SWEEPS["n_lm"], SWEEPS["per_kf"]
    X = rng.uniform(-2, 2, size=(n_lm, 3)) + [0, 0, 6]
    pose = lambda angle, t: np.array([0.0, np.sin(angle / 2), 0.0, np.cos(angle / 2), *t])  # noqa: E731
    poses = [pose(0.05 * k, [0.15 * k, 0.0, 0.02 * k]) for k in range(n)]
    poses += [pose(0.05 * k + 0.02, [0.15 * k + 0.03, 0.04, 0.02 * k]) for k in range(n)]
    kfs = []
    for T in poses:
        seen = np.sort(rng.choice(n_lm, per_kf, replace=False))
        loc = posegraph.quat_rotate(posegraph.quat_conj(T[:4]), X[seen] - T[4:])
        uv = np.stack([K_SWEEP[0] * loc[:, 0] / loc[:, 2] + K_SWEEP[2], K_SWEEP[1] * loc[:, 1] / loc[:, 2] + K_SWEEP[3]], 1)
        kfs.append(window.KeyFrame(T, uv.astype(np.float32), loc, {i: int(g) for i, g in enumerate(seen)}))
    matching.attach_descriptors(kfs, seed=7, kind="hamming", flip=0.06)
    for kf in kfs[n:]:
        kf.global_points_map = {i: g + n_lm for i, g in kf.global_points_map.items()}
    landmarks = {i: X[i % n_lm].copy() for i in range(2 * n_lm)}
    return kfs, landmarks, K_SWEEP, [(k, n + k) for k in range(n)]


def shared_ids(kfs, a, b):
    return len(set(kfs[a].global_points_map.values()) & set(kfs[b].global_points_map.values()))
