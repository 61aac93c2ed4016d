"""The outer CG's two fused steps (gmg_cg_direction_step / gmg_cg_update_step) against the calls they
replace: same bits in x, g, d and |g|^2 on vectors with odd tails, and a whole solve with the option on and off."""
import numpy as np
import pytest

from gpu_util import capi, pkg

pytestmark = pytest.mark.gpu

KEY = "disable_outer_cg_fused"


@pytest.fixture(scope="module")
def ctx():
    c = capi().Context(1)
    yield c
    c.set_option(KEY, 0)
    c.close()


def _unfused(c, x, g, d, hs):
    """Three iterations as SolverCG runs them on the calls of the vector_t interface; hs: the preconditioner's outputs."""
    out = []
    h = c.vector(x.n, hs[0])
    c.equ(d, -1.0, h)
    gh = np.float64(c.dot(g, h))  # (IEEE scalars as in the C++ loop: at n = 1 the second g.h is 0 and the third beta 0 / 0)
    for k in range(1, len(hs)):
        h.upload(hs[k])  # (stands in for h = A d)
        alpha = gh / np.float64(c.dot(d, h))
        c.add(x, alpha, d)
        c.add(g, alpha, h)
        out.append(c.dot(g, g))
        h.upload(hs[k][::-1].copy())  # (stands in for h = M^-1 g)
        beta = gh
        gh = np.float64(c.dot(g, h))
        beta = gh / beta
        c.sadd(d, beta, -1.0, h)
    h.free()
    return out


def _stepped(c, x, g, d, hs):
    out = []
    h = c.vector(x.n, hs[0])
    c.cg_direction_step(d, g, h, True)
    for k in range(1, len(hs)):
        h.upload(hs[k])
        out.append(c.cg_update_step(x, g, d, h))
        h.upload(hs[k][::-1].copy())
        c.cg_direction_step(d, g, h, False)
    h.free()
    return out


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_steps_equal_the_unfused_sequence(ctx, n):
    rng = np.random.default_rng(n)
    x0, g0 = rng.standard_normal(n), rng.standard_normal(n)
    hs = [rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4) for _ in range(4)]  # three iterations: both g.h slots are old and new once
    res = {}
    for name, run, key in (("calls", _unfused, 0), ("fused", _stepped, 0), ("key off", _stepped, 1)):
        ctx.set_option(KEY, key)
        x, g, d = ctx.vector(n, x0), ctx.vector(n, g0), ctx.vector(n)
        with np.errstate(all="ignore"):
            gg = run(ctx, x, g, d, hs)
        res[name] = (x.download(), g.download(), d.download(), np.array(gg))
        for v in (x, g, d):
            v.free()
    ctx.set_option(KEY, 0)
    assert np.isfinite(res["calls"][3][0]) and (n == 1 or np.all(res["calls"][3] > 0))
    for name in ("fused", "key off"):
        for what, a, b in zip(("x", "g", "d", "|g|^2"), res[name], res["calls"]):
            assert np.array_equal(a, b, equal_nan=True), (name, what, n)  # (NaN only at n = 1, where CG is done after one step)


def _problem(device_cg):
    """8 atoms, two adaptive cycles (the second with hanging nodes), solved on the device"""
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=1, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous",
                             cycles=2, r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0,
                             smoother="SSOR", device_cg=device_cg))
    p.set_nacl_atoms(1)
    p.run_cycle(0, on_device=True)
    p.run_cycle(1, on_device=True)
    return p


@pytest.mark.parametrize("device_cg", [False, True])
def test_whole_gmg_solve_equal_with_key_on_and_off(device_cg):
    """SolverCG_solve of the host driver (device_cg False) and gmg_cg_solve (True), GMG preconditioner"""
    p = _problem(device_cg)
    try:
        c = capi().Context.view(p.gmg_context())
        got = {}
        for key in (0, 1):
            c.set_option(KEY, key)
            r = p.solve_again()
            got[key] = (r, p.vector("solution").copy())
        c.set_option(KEY, 0)
    finally:
        p.close()
    (r1, x1), (r0, x0) = got[0], got[1]
    assert r1["cg_iterations"] >= 2, r1  # (an iteration count that exercises the direction step)
    for k in ("cg_iterations", "coarse_iterations", "starting_value", "convergence_value"):
        assert r1[k] == r0[k], (k, r1[k], r0[k])
    assert np.array_equal(x1, x0)


def test_whole_jacobi_solve_equal_with_key_on_and_off():
    """gmg_cg_solve with the Jacobi preconditioner on the same system.  (Through the C-ABI: the host driver's upload reads the
    level matrices whatever the preconditioner, and `Preconditioner = Jacobi` assembles none.)"""
    p = _problem(False)
    try:
        h = p.hierarchy()
    finally:
        p.close()
    A, b = h.system_matrix, np.asarray(h.system_rhs, dtype=np.float64)
    c = capi().Context(1)
    try:
        c.set_system_matrix(A)
        vb, vx = c.vector(A.n_rows, b), c.vector(A.n_cols)
        got = {}
        for key in (0, 1):
            c.set_option(KEY, key)
            c.set_zero(vx)
            r = c.cg_solve(vx, vb, rel_tol=1e-8, max_it=500, precond=capi().PRECOND_JACOBI)
            got[key] = (r, vx.download())
        c.set_option(KEY, 0)
    finally:
        c.close()
    (r1, x1), (r0, x0) = got[0], got[1]
    assert r1["status"] == 0 and r1["iterations"] >= 10, r1
    assert r1 == r0, (r1, r0)
    assert np.array_equal(x1, x0)
