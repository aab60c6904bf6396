"""Windows on the edges of the Schur reduction, a restated plan geometry and a reference reduced system (test
infrastructure).

The step tests' windows (refstep.WINDOWS) sit on the edges of the reduced *solve*. The windows here sit on the edges
of the stage before it: the plan's classification of points (tiled, overflow, gauge-only), its tiles, chunks,
back-substitution chunks and camera sub-segments (csrc/ba_plan.cpp), and the kernels that consume them. They are
synthetic.make_problem windows whose observation arrays are then edited: observations dropped by mask, noisy copies
appended. Tracks are contiguous camera ranges, so a mask gives any span and count and a copy gives a repeated link.

* ``WINDOWS`` / ``window(name)``     the windows (cached; callers must not modify them)
* ``reference(name, radius)``        refstep.reference's tuple for them
* ``geometry(prob, tile_pts, subseg)``  what the plan of a window must be, restated in plain Python from the
                                     comments of ba_plan.h and ba_kernels.h (no code shared with ba_plan.cpp)
* ``schur_system(prob, opts, radius)``  the scaled, damped reduced system refstep.schur_step solves, rounded to f64
"""
from __future__ import annotations

import numpy as np

import refstep
from refstep import LD, EPS64

# the limits of the Schur stage (ba_kernels.h) as the restatement states them
TILE_WIN = 12      # active cameras per tile window
CHUNK_PTS = 32     # points per Schur chunk
CHUNK_OBS = 256    # observations per Schur chunk; a point with more is an overflow point
BS_PTS = 128       # points per back-substitution chunk
BS_OBS = 1024      # observations per back-substitution chunk (a single point may exceed)

# MIBA_TILE_PTS of the short400 runs and of the plan comparison. short400's tracks are too short for the camera
# window to cut a tile, so a tile's last chunk has tile_pts mod 32 points: 1, 3, 31 and 32 from the first six values
# (K = 3 and 9 of the MFMA product, not multiples of 4), and 34 and 37 add last chunks of 2 and 5 points (K = 6, 15)
TILE_PTS = (1, 3, 31, 32, 33, 97, 34, 37)
SUBSEGS = (64, 256)
RADII = (1e4, 1e-2)

BASE = dict(n_cams=16, n_points=192, obs_per_point=14, seed=914)  # tracks start on camera 0, 1 or 2; gauge 0


# ------------------------------------------------------------------------------------------------ sculpting
def _edit(p, keep=None, copies=(), seed=0):
    """``p`` with the observations of ``keep`` (a mask; default all), then one noisy copy per entry of ``copies``
    (indices into p's observations, repeats allowed): the pixel moved by N(0, 1), the depth by a factor
    1 + N(0, 0.01), as synthetic.make_problem's duplicate links are. float32-valued windows stay float32-valued."""
    from miba.capi import ProblemArrays
    keep = np.ones(p.n_obs, bool) if keep is None else np.asarray(keep, bool)
    copies = np.asarray(copies, dtype=np.int64)
    rng = np.random.default_rng(seed)
    uv_c = p.obs_uv[copies] + rng.normal(0.0, 1.0, (len(copies), 2))
    dep_c = p.obs_depth[copies] * (1.0 + rng.normal(0.0, 0.01, len(copies)))
    f32 = bool(np.all(p.obs_uv.astype(np.float32) == p.obs_uv) and np.all(p.obs_depth.astype(np.float32) == p.obs_depth))
    if f32:
        uv_c, dep_c = uv_c.astype(np.float32).astype(np.float64), dep_c.astype(np.float32).astype(np.float64)
    return ProblemArrays(p.cams.copy(), p.points.copy(), p.intr.copy(), p.intr_prior.copy(),
                         np.concatenate([p.obs_cam[keep], p.obs_cam[copies]]),
                         np.concatenate([p.obs_pt[keep], p.obs_pt[copies]]),
                         np.concatenate([p.obs_uv[keep], uv_c]), np.concatenate([p.obs_depth[keep], dep_c]),
                         p.fixed_cam)


def _obs_of(p, pt, cam=None):
    m = p.obs_pt == pt
    if cam is not None:
        m &= p.obs_cam == cam
    return np.nonzero(m)[0]


def _spans(**kw):
    """Point i keeps the first 1 + i % 14 cameras of its 14-camera track."""
    from miba import synthetic
    p = synthetic.make_problem(**BASE, **kw)
    first = np.full(p.n_points, p.n_cams, np.int64)
    np.minimum.at(first, p.obs_pt, p.obs_cam)
    return _edit(p, p.obs_cam - first[p.obs_pt] < 1 + p.obs_pt % 14)


def _holes():
    """spans without the interior observations of every third point: the first and the last camera stay, and the
    second one too on every other such point (2 or 3 observations carry the span)."""
    p = _spans()
    first = np.full(p.n_points, p.n_cams, np.int64)
    last = np.full(p.n_points, -1, np.int64)
    np.minimum.at(first, p.obs_pt, p.obs_cam)
    np.maximum.at(last, p.obs_pt, p.obs_cam)
    rel = p.obs_cam - first[p.obs_pt]
    edge = (rel == 0) | (p.obs_cam == last[p.obs_pt]) | ((rel == 1) & (p.obs_pt % 2 == 1))
    return _edit(p, (p.obs_pt % 3 != 0) | edge)


# points of `spans` by what they are: 70 observes camera 1 alone (active span 1), 67 cameras 1..12 (span 12),
# 68 cameras 1..13 (span 13: overflow), 5 cameras 0..5 and 12 cameras 0..12 (gauge + 12 active: tiled)
PT_SPAN1, PT_SPAN12, PT_SPAN13, PT_GAUGE6, PT_GAUGE13 = 70, 67, 68, 5, 12
CHUNK_CUT_PTS = (2, 3, 4, 5, 6)  # neighbours in the tiled order, inflated to 60 observations each


def _dup_active():
    p = _spans()
    return _edit(p, copies=[_obs_of(p, PT_SPAN1, 1)[0], _obs_of(p, PT_SPAN12, 7)[0]], seed=1)


def _dup_gauge():
    p = _spans()
    return _edit(p, copies=[_obs_of(p, PT_GAUGE6, 0)[0], _obs_of(p, PT_GAUGE13, 0)[0]], seed=2)


def _obs_n(extra):
    p = _spans()
    return _edit(p, copies=np.repeat(_obs_of(p, PT_GAUGE6, 0)[0], extra), seed=3)


def _chunk_cut():
    p = _spans()
    cp = np.concatenate([np.repeat(_obs_of(p, i, 0)[0], 60 - len(_obs_of(p, i))) for i in CHUNK_CUT_PTS])
    return _edit(p, copies=cp, seed=4)


def _bs_long():
    p = _spans()
    return _edit(p, copies=np.tile(_obs_of(p, PT_SPAN13), 79), seed=5)


def _all_overflow():
    """Every point with an observation of an active camera gets a copy of its last such observation."""
    p = _spans()
    act = np.nonzero(p.obs_cam != p.fixed_cam)[0]
    last = {}
    for k in act:
        last[int(p.obs_pt[k])] = int(k)
    return _edit(p, copies=sorted(last.values()), seed=6)


def _gauge_only():
    """The points whose track starts on the gauge camera keep that observation alone (even points) or that one and
    camera 1's (odd points)."""
    p = _spans()
    first = np.full(p.n_points, p.n_cams, np.int64)
    np.minimum.at(first, p.obs_pt, p.obs_cam)
    on_gauge = first[p.obs_pt] == 0
    return _edit(p, ~on_gauge | (p.obs_cam == 0) | ((p.obs_cam == 1) & (p.obs_pt % 2 == 1)))


def _short400():
    from miba import synthetic
    return synthetic.make_problem(14, 400, (2, 4), seed=77)


WINDOWS = {
    "spans": _spans,
    "holes": _holes,
    "dup_active": _dup_active,
    "dup_gauge": _dup_gauge,
    "obs256": lambda: _obs_n(250),
    "obs257": lambda: _obs_n(251),
    "chunk_cut": _chunk_cut,
    "bs_long": _bs_long,
    "all_overflow": _all_overflow,
    "gauge_only": _gauge_only,
    "short400": _short400,
    "spans_f32": lambda: _spans(sensor_f32=True),
}
# the windows of the variant matrix (test_gpu_schur.py)
VARIANT_WINDOWS = ("spans", "holes", "obs256", "obs257", "chunk_cut", "bs_long", "dup_active", "short400")
# MIBA_TILE_PTS of a run that does not vary it: half a chunk on the sculpted windows (the tiles of small windows),
# a whole chunk on short400
DEFAULT_TILE_PTS = {n: 16 for n in WINDOWS}
DEFAULT_TILE_PTS["short400"] = 32

_cache = {}


def window(name):
    """The window ``name`` (cached; callers must not modify it)."""
    if ("w", name) not in _cache:
        _cache[("w", name)] = WINDOWS[name]()
    return _cache[("w", name)]


def reference(name, radius=1e4):
    """(window, schur_step, oracle.lm_step, the oracle's own accept decision) of ``name`` at ``radius``, cached: the
    tuple of refstep.reference."""
    from oracle import oracle
    key = ("r", name, float(radius))
    if key not in _cache:
        p = window(name)
        ref = refstep.schur_step(p, None, radius)
        orc = oracle.lm_step(p, None, radius)
        _, tr = oracle.solve_trace(p.copy(), oracle.default_options(max_num_iterations=1,
                                                                    initial_trust_region_radius=radius,
                                                                    **refstep.NO_TOL))
        _cache[key] = (p, ref, orc, int(tr[1][6]))
    return _cache[key]


def schur_system(prob, opts=None, radius: float = 0.0):
    """(S, rhs) of the scaled, damped reduced system of refstep.schur_step — active cameras in increasing order,
    six rows each, then the four intrinsics — assembled in extended precision, rounded to f64 on return."""
    S, rhs, _ = refstep.schur_reduce(refstep._Lin(prob, opts, radius))
    return S.astype(np.float64), rhs.astype(np.float64)


def system_err(S, rhs, S_ref, rhs_ref):
    """(max_ij |S - S_ref|_ij / sqrt(S_ref,ii S_ref,jj), max_i |rhs - rhs_ref|_i / sqrt(S_ref,ii))."""
    d = np.sqrt(np.diag(S_ref))
    return (float((np.abs(S - S_ref) / np.outer(d, d)).max()), float((np.abs(rhs - rhs_ref) / d).max()))


def longest_camera_sum(prob) -> int:
    """The largest admissible observation count of an active camera: the longest sum behind one entry of a camera
    block of S."""
    adm = prob.obs_depth > 1e-15
    cnt = np.bincount(prob.obs_cam[adm], minlength=prob.n_cams)
    if 0 <= prob.fixed_cam < prob.n_cams:
        cnt[prob.fixed_cam] = 0
    return int(cnt.max())


# ------------------------------------------------------------------------------------------------ the geometry
def geometry(prob, tile_pts, subseg, chunk_obs=CHUNK_OBS, tile_win=TILE_WIN) -> dict:
    """What the plan of ``prob`` must be at a fixed MIBA_TILE_PTS and MIBA_SUBSEG, as lists of ints.

    Admissible observations have depth > 1e-15. Active cameras: those with an admissible observation, without the
    gauge, numbered in increasing order. Per observed point: pmin / pmax, the first / last active camera (active
    index) it observes; class 2 (gauge-only) when it observes none, class 1 (overflow) when two of its observations
    fall on the same active camera, when pmax - pmin + 1 > TILE_WIN or when it has more than CHUNK_OBS
    observations (the gauge's counted), class 0 (tiled) otherwise. The active point order: tiled points by pmin,
    then overflow points by pmin, ties in point order, then the gauge-only points in point order. A tile takes
    tiled points in that order while it has fewer than tile_pts and the next one's pmax stays inside [base, base +
    TILE_WIN), base the pmin of its first point; its span reaches to the largest pmax taken. Its chunks take <=
    CHUNK_PTS points and <= CHUNK_OBS observations. Back-substitution chunks run over all active points: <= BS_PTS
    points, <= BS_OBS observations unless a single point. Every camera with admissible observations (the gauge too)
    cuts its camera-major range into ceil(count / subseg) near-equal sub-segments."""
    adm = np.nonzero(prob.obs_depth > 1e-15)[0]
    nc, npt = prob.n_cams, prob.n_points
    cam = [int(c) for c in prob.obs_cam[adm]]
    pt = [int(q) for q in prob.obs_pt[adm]]
    cam_cnt = [0] * nc
    for c in cam:
        cam_cnt[c] += 1
    ac_cam = [c for c in range(nc) if cam_cnt[c] > 0 and c != prob.fixed_cam]
    cam_ac = {c: a for a, c in enumerate(ac_cam)}
    nac = len(ac_cam)
    seen = [[] for _ in range(npt)]  # per point: the active index (-1: gauge) of each admissible observation
    for c, q in zip(cam, pt):
        seen[q].append(cam_ac.get(c, -1))
    pclass, pmin, pmax = [-1] * npt, [None] * npt, [None] * npt
    for q in range(npt):
        if not seen[q]:
            continue
        act = [a for a in seen[q] if a >= 0]
        if not act:
            pclass[q] = 2
            continue
        pmin[q], pmax[q] = min(act), max(act)
        dup = len(set(act)) < len(act)
        pclass[q] = 1 if dup or pmax[q] - pmin[q] + 1 > tile_win or len(seen[q]) > chunk_obs else 0
    tiled = sorted((q for q in range(npt) if pclass[q] == 0), key=lambda q: (pmin[q], q))
    ovf = sorted((q for q in range(npt) if pclass[q] == 1), key=lambda q: (pmin[q], q))
    gauge = [q for q in range(npt) if pclass[q] == 2]
    pt_idx = tiled + ovf + gauge
    cnt = [len(seen[q]) for q in pt_idx]
    pt_ptr = [0]
    for n in cnt:
        pt_ptr.append(pt_ptr[-1] + n)
    # tiles and chunks
    tile_base, tile_span, tile_chunk, chunk_ap = [], [], [0], [0]
    i = 0
    while i < len(tiled):
        base = pmin[tiled[i]]
        j = i
        while j < len(tiled) and j - i < tile_pts and pmax[tiled[j]] < base + tile_win:
            j += 1
        c0 = i
        while c0 < j:
            c1, nob = c0, 0
            while c1 < j and c1 - c0 < CHUNK_PTS and nob + cnt[c1] <= chunk_obs:
                nob += cnt[c1]
                c1 += 1
            assert c1 > c0
            chunk_ap.append(c1)
            c0 = c1
        tile_base.append(base)
        tile_span.append(max(pmax[q] for q in tiled[i:j]) - base + 1)
        tile_chunk.append(len(chunk_ap) - 1)
        i = j
    n_ovf_obs = sum(1 for q in ovf for a in seen[q] if a >= 0)
    # back-substitution chunks
    bs_chunk, a = [0], 0
    while a < len(pt_idx):
        b = a + 1
        while b < len(pt_idx) and b - a < BS_PTS and pt_ptr[b + 1] - pt_ptr[a] <= BS_OBS:
            b += 1
        bs_chunk.append(b)
        a = b
    # camera sub-segments
    seg_ptr, seg_cam, seg_ac, ac_seg, start = [0], [], [], [0] * (2 * max(nac, 1)), 0
    for c in range(nc):
        n = cam_cnt[c]
        if n == 0:
            continue
        nseg = -(-n // subseg)
        if c in cam_ac:
            ac_seg[2 * cam_ac[c]], ac_seg[2 * cam_ac[c] + 1] = len(seg_cam), len(seg_cam) + nseg
        for k in range(1, nseg + 1):
            seg_cam.append(c)
            seg_ac.append(cam_ac.get(c, -1))
            seg_ptr.append(start + n * k // nseg)
        start += n
    # first co-visible active camera
    fc = list(range(nac))
    for q in pt_idx:
        for a in seen[q]:
            if a >= 0:
                fc[a] = min(fc[a], pmin[q])
    return dict(nac=nac, ac_cam=ac_cam, cam_cnt=cam_cnt, n_tiled=len(tiled), n_ovf=len(ovf), n_gauge=len(gauge),
                pclass=pclass, pmin=[-1 if v is None else v for v in pmin], pmax=[-1 if v is None else v for v in pmax],
                pt_idx=pt_idx, pt_ptr=pt_ptr, tile_base=tile_base, tile_span=tile_span, tile_chunk=tile_chunk,
                chunk_ap=chunk_ap, n_ovf_obs=n_ovf_obs, bs_chunk=bs_chunk, seg_ptr=seg_ptr, seg_cam=seg_cam,
                seg_ac=seg_ac, ac_seg=ac_seg, fc=fc)


def envelope_tiles(fc) -> int:
    """16x16 tiles of the envelope of S (6 rows per active camera from the column of its first co-visible camera,
    the intrinsics rows and the padding from column 0), block rows of 16."""
    nac = len(fc)
    npad = (6 * nac + 4 + 15) // 16 * 16
    first = [6 * fc[r // 6] // 16 if r < 6 * nac else 0 for r in range(npad)]
    return sum(i - min(first[16 * i: 16 * i + 16]) + 1 for i in range(npad // 16))


def sw_launch_blocks(geo) -> int:
    """Workgroups of the small-window Schur launch: the tiles, the intrinsics term, the camera sub-segments, 256
    non-tiled points each, the envelope tiles. The launch is taken (lin_path 1 under MIBA_SW=2) up to 256."""
    non_tiled = geo["n_ovf"] + geo["n_gauge"]
    return len(geo["tile_base"]) + 1 + len(geo["seg_cam"]) + -(-non_tiled // 256) + envelope_tiles(geo["fc"])
