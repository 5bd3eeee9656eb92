"""The two files of the fused hex-8 assembly (csrc/hex8_thermal.hip, csrc/hex8_elasticity.hip) each own a copy of the reference tables in
constant memory, uploaded by their own mfem_hex8_upload_tables behind their own cache of the Gauss rule last uploaded.  One process
alternates between the physics and between the rules, so that each file re-uploads while the other keeps its own rule: thermal with 2
Gauss points per direction, elasticity with 3, thermal 3, elasticity 2, thermal 1 and 4 (the tile kernels), elasticity 4, then the first
two again.  Every K and R against the oracle at the tolerances of test_gpu_thermal.py (K 1e-13, R 1e-12) and
test_gpu_elasticity_edges.py (K 2e-13, R 1e-12); a repeated call gives the bits of the first call of its kind."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = (3, 4, 2)
ITG = {1: 1, 2: 3, 3: 5, 4: 7}  # Gauss points per direction -> an integration order with that rule
SEQUENCE = [("thermal", 2), ("elasticity", 3), ("thermal", 3), ("elasticity", 2), ("thermal", 1), ("thermal", 4), ("elasticity", 4),
            ("thermal", 2), ("elasticity", 3)]


def test_each_file_keeps_its_own_tables(mf):
    import torch
    import test_gpu_elasticity_edges as el
    import test_gpu_thermal as th

    def distort(c):
        return el._distort(c, el.X)

    pen, tra = "x0|z1", "y1|x0"
    oracles = {}
    for kind, ng in dict.fromkeys(SEQUENCE):
        if kind == "thermal":
            od = th._oracle_domain(el.X, N, ITG[ng], distort)
            od.update_time()
            od.K_linear_func()
            od.x_star[:] = 300.0 + 20.0 * np.random.default_rng(1).standard_normal(od.basicfield_size)
            od.K_nonlinear_func()
        else:
            od = el._oracle(el.X, N, pen, tra, itg=ITG[ng])
        assert od.elgeo.integral_weights.shape[0] == ng ** 3
        oracles[kind, ng] = od
    coords = oracles["thermal", 2].mesh.coords
    assert np.array_equal(coords, oracles["elasticity", 3].mesh.coords)  # one distorted brick

    first = {}
    for step, (kind, ng) in enumerate(SEQUENCE):
        od = oracles[kind, ng]
        brick = el._brick(mf, el.X, N, ITG[ng], coords)
        xs = torch.tensor(od.x_star, device="cuda")
        if kind == "thermal":
            A = brick.pattern(1)
            s = torch.full((brick.ncp,), th.SRC, dtype=torch.float64, device="cuda")
            K = brick.assemble_thermal(A, th.K_COND, th.H, th.TENV, 0x3F).cpu().numpy()
            R = brick.residual_thermal(xs, th.K_COND, th.H, th.TENV, 0x3F, s=s).cpu().numpy()
            k_tol, r_tol = 1e-13, 1e-12
        else:
            A = brick.pattern(3)
            K = brick.assemble_elasticity(A, el.LAM, el.MU, el.TAU_REF, el._bits(mf, pen)).cpu().numpy()
            R = brick.residual_elasticity(xs, el.LAM, el.MU, el.TAU_REF, el._bits(mf, pen), el._bits(mf, tra), el.SIG6).cpu().numpy()
            k_tol, r_tol = el.K_TOL, el.R_TOL
        el._close(f"step {step} {kind} ng={ng} K", K, od.K_linear, k_tol)
        el._close(f"step {step} {kind} ng={ng} R", R, od.residue, r_tol)
        if (kind, ng) in first:
            assert np.array_equal(K, first[kind, ng][0]) and np.array_equal(R, first[kind, ng][1]), f"step {step}: {kind} ng={ng} gives other bits than its first call"
        else:
            first[kind, ng] = (K, R)
    assert len(first) == len(SEQUENCE) - 2
