"""The sweep windows of the wide-window tests (test infrastructure): synthetic.make_sweep_problem, 12 points per
camera, two sweeps. Their references are refstep's, cached here like refstep.reference caches its own windows'."""
import refstep
from oracle import oracle

# 22 cameras, 2 x 4 observations per point: camera band 14, npad 144 (a ragged last 64-block);
# 42 cameras, 2 x 5: camera band 25, npad 256 (four full blocks: the default selection's threshold)
SWEEPS = {
    "sweep22": dict(n_cams=22, n_points=12 * 22, obs_per_pass=4, passes=2, seed=801),
    "sweep42": dict(n_cams=42, n_points=12 * 42, obs_per_pass=5, passes=2, seed=802),
}

_cache = {}


def window(name):
    """The sweep window ``name`` (cached; callers must not modify it)."""
    if ("w", name) not in _cache:
        from miba import synthetic
        _cache[("w", name)] = synthetic.make_sweep_problem(**SWEEPS[name])
    return _cache[("w", name)]


def reference(name, radius=1e4):
    """(window, schur_step, oracle.lm_step, the oracle's own accept decision) at ``radius``, cached; a refstep window
    name is passed on to refstep.reference."""
    if name not in SWEEPS:
        return refstep.reference(name, radius)
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


def npad(prob) -> int:
    """Padded size of the window's reduced system."""
    ac_cam, _ = refstep.first_covisible(prob)
    return (6 * len(ac_cam) + 4 + 15) // 16 * 16
