"""The windows of tests/refschur.py on the CPU: the references carry them, and they sit on the edges they name.

On every window, at the default radius 1e4 and under heavy damping (1e-2): the oracle's step is within
tol = 8 cond(S) eps of refstep.schur_step (so test_gpu_schur.py never runs against a window on which reference and
oracle disagree), and refstep.qr_step — no Schur complement, no normal equations — agrees with schur_step as closely
as on the windows of test_refstep.py. The expected class counts guard against a later edit of the generator or of the
sculpting silently moving a window off its edge."""
import numpy as np
import pytest

import refschur
import refstep
from oracle import oracle

CASES = [(n, r) for n in refschur.WINDOWS for r in refschur.RADII]


@pytest.mark.parametrize("name,radius", CASES)
def test_oracle_step_within_tol_of_reference(name, radius):
    p, ref, orc, accepted = refschur.reference(name, radius)
    tol = refstep.step_tol(ref.cond)
    err = refstep.rel_err(orc, ref)
    print(f"ORACLE {name} radius={radius:g} nac={len(ref.ac_cam)} cond={ref.cond:.3g} tol={tol:.2e} "
          f"err cams={err['cams']:.1e} intr={err['intr']:.1e} pts={err['pts']:.1e}")
    assert max(err.values()) <= tol, (err, tol)
    assert abs(orc["model_cost_change"] - ref.model_cost_change) <= tol * ref.model_cost_change
    assert accepted == 1


@pytest.mark.parametrize("name,radius", CASES)
def test_qr_and_schur_references_agree(name, radius):
    p, s = refschur.reference(name, radius)[:2]
    q = refstep.qr_step(p, None, radius)
    err = refstep.rel_err(q, s)
    print(f"REF {name} radius={radius:g} cond={s.cond:.3g} qr-schur {err}")
    assert max(err.values()) <= 1e-12, err
    assert abs(q.model_cost_change - s.model_cost_change) <= 1e-13 * abs(s.model_cost_change)
    assert s.model_cost_change > 0


@pytest.mark.parametrize("name", sorted(refschur.WINDOWS))
def test_schur_system_is_what_the_oracle_assembles(name):
    """refschur.schur_system against the f64 oracle's reduced system (which holds the gradient side, S y = -rhs):
    the same matrix to the oracle's rounding, so the two share layout, scaling and damping."""
    p = refschur.window(name)
    for radius in (1e4, 3.0):
        S, rhs = refschur.schur_system(p, None, radius)
        So, ro = oracle.reduced_system(p, oracle.default_options(), radius)
        e_s, e_r = refschur.system_err(So, -ro, S, rhs)
        print(f"SYS {name} radius={radius:g} oracle S={e_s:.1e} rhs={e_r:.1e} "
              f"m eps={refschur.longest_camera_sum(p) * refschur.EPS64:.1e}")
        assert e_s <= 1e-10 and e_r <= 1e-10


# window: (tiled, overflow, gauge-only) points
CLASS_COUNTS = {
    "spans": (165, 22, 5), "holes": (165, 22, 5), "dup_active": (163, 24, 5), "dup_gauge": (165, 22, 5),
    "obs256": (165, 22, 5), "obs257": (164, 23, 5), "chunk_cut": (165, 22, 5), "bs_long": (165, 22, 5),
    "all_overflow": (0, 187, 5), "gauge_only": (142, 18, 32), "short400": (400, 0, 0), "spans_f32": (165, 22, 5),
}


@pytest.mark.parametrize("name", sorted(refschur.WINDOWS))
def test_windows_keep_their_classes(name):
    p = refschur.window(name)
    g = refschur.geometry(p, refschur.DEFAULT_TILE_PTS[name], 256)
    assert (g["n_tiled"], g["n_ovf"], g["n_gauge"]) == CLASS_COUNTS[name]
    assert g["nac"] == p.n_cams - 1 and p.fixed_cam == 0
    assert p.n_obs <= 2600


def test_windows_reach_their_edges():
    geo = {n: refschur.geometry(refschur.window(n), refschur.DEFAULT_TILE_PTS[n], 256) for n in refschur.WINDOWS}

    def span(g, q):
        return g["pmax"][q] - g["pmin"][q] + 1

    def chunk_obs(g):
        return [g["pt_ptr"][b] - g["pt_ptr"][a] for a, b in zip(g["chunk_ap"], g["chunk_ap"][1:])]

    g = geo["spans"]
    tiled = [q for q in range(192) if g["pclass"][q] == 0]
    assert {span(g, q) for q in tiled} == set(range(1, 13))
    assert {span(g, q) for q in range(192) if g["pclass"][q] == 1} == {13, 14}
    # a track from the gauge camera over 13 cameras is 12 active cameras wide: tiled
    assert g["pclass"][refschur.PT_GAUGE13] == 0 and span(g, refschur.PT_GAUGE13) == 12
    assert set(refschur.geometry(refschur.window("spans"), 1, 256)["tile_span"]) == set(range(1, 13))
    g, p = geo["holes"], refschur.window("holes")
    cnt = np.bincount(p.obs_pt, minlength=192)
    assert any(span(g, q) == 12 and cnt[q] in (2, 3) for q in range(192) if g["pclass"][q] == 0)
    assert any(span(g, q) == 13 and cnt[q] in (2, 3) for q in range(192) if g["pclass"][q] == 1)
    g = geo["dup_active"]
    assert g["pclass"][refschur.PT_SPAN1] == 1 and g["pclass"][refschur.PT_SPAN12] == 1
    assert span(g, refschur.PT_SPAN1) == 1 and span(g, refschur.PT_SPAN12) == 12
    g = geo["dup_gauge"]
    assert g["pclass"][refschur.PT_GAUGE6] == 0 and g["pclass"][refschur.PT_GAUGE13] == 0
    g = geo["obs256"]
    assert g["pclass"][refschur.PT_GAUGE6] == 0 and chunk_obs(g).count(refschur.CHUNK_OBS) == 1
    a = g["pt_idx"].index(refschur.PT_GAUGE6)
    assert g["pt_ptr"][a + 1] - g["pt_ptr"][a] == 256 and a in g["chunk_ap"] and a + 1 in g["chunk_ap"]
    g = geo["obs257"]
    assert g["pclass"][refschur.PT_GAUGE6] == 1 and span(g, refschur.PT_GAUGE6) == 5
    g = geo["chunk_cut"]
    ends = {g["chunk_ap"][c] for c in g["tile_chunk"]}
    assert any(b not in ends and b - a < refschur.CHUNK_PTS for a, b in zip(g["chunk_ap"], g["chunk_ap"][1:]))
    g = geo["bs_long"]
    assert max(g["pt_ptr"][b] - g["pt_ptr"][a] for a, b in zip(g["bs_chunk"], g["bs_chunk"][1:])) == 1040
    assert g["pclass"][refschur.PT_SPAN13] == 1
    g = geo["all_overflow"]
    assert g["tile_base"] == [] and g["n_tiled"] == 0
    g, p = geo["gauge_only"], refschur.window("gauge_only")
    cnt = np.bincount(p.obs_pt, minlength=192)
    assert g["n_gauge"] == 32 and all(cnt[q] == 1 for q in range(192) if g["pclass"][q] == 2)
    assert sum(1 for q in range(64) if g["pclass"][q] == 0 and cnt[q] == 2 and span(g, q) == 1) == 32
    # short400: tiles whose last chunk has 1, 2, 3 and 5 points (K = 3, 6, 9, 15) over the MIBA_TILE_PTS list
    last = set()
    for t in refschur.TILE_PTS:
        g = refschur.geometry(refschur.window("short400"), t, 256)
        last |= {g["chunk_ap"][c] - g["chunk_ap"][c - 1] for c in g["tile_chunk"][1:]}
        if t > 32:
            assert any(b - a > 1 for a, b in zip(g["tile_chunk"], g["tile_chunk"][1:]))  # several chunks per tile
    assert {1, 2, 3, 5} <= last, last
    assert refschur.window("spans_f32").obs_uv.astype(np.float32).astype(np.float64).tolist() == \
        refschur.window("spans_f32").obs_uv.tolist()
