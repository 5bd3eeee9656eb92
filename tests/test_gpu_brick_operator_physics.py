"""GPU: the four physics of the matrix-free brick operator behind one ops table (csrc/brick_operator.hip; the physics rows:
csrc/brick_operator_physics.h; the hex-8 thermal kernels: csrc/brick_operator_thermal.hip) keep the bits and the answers of the commit before the
table existed.  Everything here is compared with files recorded ON THAT COMMIT by record(), never with what the present code gives:
  tests/golden/brick_operator_physics_sha256.json    SHA-256 of mul_ (alpha = 1, beta = 0 and alpha = -0.5, beta = 2 on a non-zero y), diagonal(),
        mfem_debug_brick_operator_apply_dot (y, the partial sums, their number), mfem_debug_brick_operator_signed_diagonal (the three physics that
        have one) and residual() (hex-27 elasticity); iterations and final_res of one cg_ + Pr_Jacobi_ solve (the bound path: dsc is set)
  tests/golden/brick_operator_physics_refusals.json  return code and error text of the four multigrid creates, the two set-params and the
        elasticity residual on a handle of each physics and on a mesh operator's
Shapes: the smallest on which every launcher takes each of its paths (CASES).  Coordinates are moved by a formula, vectors come from numpy's seeded
generator.  The face kernels launch: Robin on x1 and Nitsche on x0 (thermal), penalty faces x0 and x1 (elasticity).

An error text of MFEM_REQUIRE is "<file>:<line>: <message> (<condition>)": the file, the line and the spelling of the condition are where the
check stands in the source, which a split of a file moves by construction; of those texts the message is compared, in full.  A refusal's text
(MFEM_ERR_UNSUPPORTED) carries no source position and is compared whole."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_SHA = os.path.join(ROOT, "tests", "golden", "brick_operator_physics_sha256.json")
GOLDEN_REFUSALS = os.path.join(ROOT, "tests", "golden", "brick_operator_physics_refusals.json")
XB = (1.0, 1.5, 0.75)
K_COND, H, TENV, H_PEN = 0.6, 25.0, 293.15, 1000.0
LAM, MU, TAU = 0.5769, 0.3846, 1.0
X0, X1, Z1 = 1 << 4, 1 << 2, 1 << 5
SIG6 = (0.01, -0.004, 0.006, 0.003, -0.002, 0.005)
# name, physics, interpolation order, itg_order (the rule has itg // 2 + 1 points), element counts
CASES = [
    ("hex8-thermal-sweep", "thermal", 1, 3, (6, 16, 5)),      # 2-point rule: the sweep; 17 lattice points in j cross its 15-point tile
    ("hex8-thermal-tiles-ng1", "thermal", 1, 1, (6, 16, 5)),  # 1- and 4-point rules: the 4 x 4 x 8 tiles
    ("hex8-thermal-tiles-ng4", "thermal", 1, 7, (6, 16, 5)),
    ("hex8-elasticity", "elasticity", 1, 3, (6, 16, 5)),
    ("hex27-thermal", "hex27", 2, 5, (5, 9, 3)),              # 9 elements in j cross the 8-element tile; a sweep longer than B27_LMIN
    ("hex27-elasticity", "elasticity_hex27", 2, 5, (5, 9, 3)),
]
CASE_IDS = [c[0] for c in CASES]
SIGNED = {"thermal", "elasticity", "hex27"}
CREATES = ["mfem_brick_multigrid_create", "mfem_brick_multigrid_create_nonsymmetric", "mfem_brick_multigrid_create_elasticity",
           "mfem_brick_multigrid_create_hex27"]
KINDS = ["thermal", "elasticity", "hex27", "elasticity_hex27", "mesh"]


def _operator(mf, physics, brick, faces=True):
    if physics in ("thermal", "hex27"):
        make = brick.thermal_operator if physics == "thermal" else brick.thermal_operator_hex27
        return make(K_COND, H, TENV, X1, fixed_faces=X0, h_penalty=H_PEN) if faces else make(K_COND, H, TENV, X0 | X1)
    if physics == "elasticity":
        return brick.elasticity_operator(LAM, MU, TAU, X0 | X1)
    return brick.elasticity_operator_hex27(LAM, MU, TAU, X0 | X1, Z1, SIG6)


def _distorted_brick(mf, order, itg, n):
    import torch

    brick = mf.make_Brick(XB, n, order, itg)
    c = [brick.coords_view(d).clone() for d in range(3)]
    brick.coords_view(0).add_(0.03 * torch.sin(3 * c[1]) * torch.cos(2 * c[2]))
    brick.coords_view(1).add_(0.02 * torch.sin(2 * c[0] + c[2]))
    brick.coords_view(2).add_(0.025 * c[0] * c[1])
    return brick


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def _dev(a):
    import torch

    return torch.tensor(a, device="cuda")


def digests(mf, case):
    """what record() wrote on the parent commit and the test computes again"""
    import torch
    from metafem_jl_amd import _lib

    _, physics, order, itg, n = case
    brick = _distorted_brick(mf, order, itg, n)
    op = _operator(mf, physics, brick)
    rng = np.random.default_rng(11)
    x, y0, w = (_dev(rng.uniform(-1.0, 1.0, op.n)) for _ in range(3))
    out = {"n_unknowns": op.n}
    count = int(_lib.lib.mfem_debug_brick_operator_count())
    out["mul"] = _sha(op.mul_(torch.empty_like(x), x))
    out["count_after_one_product"] = int(_lib.lib.mfem_debug_brick_operator_count()) - count
    out["mul_alpha_beta"] = _sha(op.mul_(y0.clone(), x, -0.5, 2.0))
    out["diagonal"] = _sha(op.diagonal())
    y, partials, npart = y0.clone(), torch.zeros(4096, dtype=torch.float64, device="cuda"), C.c_int32(-1)
    count = int(_lib.lib.mfem_debug_brick_operator_count())
    _lib.check(_lib.lib.mfem_debug_brick_operator_apply_dot(op.ctx._h, op._h, x.data_ptr(), y.data_ptr(), -0.5, 2.0, w.data_ptr(), partials.data_ptr(),
                                                          C.byref(npart)))
    out["count_after_one_apply_dot"] = int(_lib.lib.mfem_debug_brick_operator_count()) - count
    out["apply_dot_y"], out["apply_dot_n_partials"] = _sha(y), npart.value
    out["apply_dot_partials"] = _sha(partials[:max(npart.value, 0)])
    d = torch.zeros(op.n, dtype=torch.float64, device="cuda")
    rc = _lib.lib.mfem_debug_brick_operator_signed_diagonal(op.ctx._h, op._h, d.data_ptr())
    if physics in SIGNED:
        _lib.check(rc)
        out["signed_diagonal"] = _sha(d)
    else:
        out["signed_diagonal_rc"], out["signed_diagonal_message"] = rc, _message(rc, _lib.lib.mfem_last_error().decode())
    if physics == "elasticity_hex27":
        out["residual"] = _sha(op.residual(x))
    # the bound path (a solve binds the column scaling: dsc is set in every product); without the Nitsche term, which cg_ is not made for
    sym = _operator(mf, physics, brick, faces=False)
    b = sym.mul_(torch.empty_like(x), x)
    sol, st = mf.iterative_Solve(sym, None, b, 1e-8 * float(b.abs().max()), Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=2000, max_pass=1)
    out["cg_jacobi"] = {"iterations": int(st.iterations), "final_res": float(st.final_res).hex(), "converged": int(st.converged), "x": _sha(sol)}
    return out


def _message(rc, text):
    """the comparable part of an error text (the module's docstring says why): MFEM_REQUIRE's message without the source position in front and the
    stringified condition behind; anything else whole"""
    if rc != -1:
        return text
    text = re.sub(r"^[\w./-]+:\d+: ", "", text)
    if text.endswith(")"):
        depth = 0
        for i in range(len(text) - 1, -1, -1):
            depth += (text[i] == ")") - (text[i] == "(")
            if depth == 0:
                return text[:i].rstrip()
    return text


def _mesh_operator(mf, ctx):
    from metafem_jl_amd import element, generic as G, mesh as pm, physics as P

    space = element.classical_space(3, "Lagrange", 1, 3, shape="CUBE")
    vert, conn = pm.make_Brick((1.0, 1.0, 1.0), (2, 2, 2), "CUBE")
    msh = pm.mesh_Classical(vert, conn, space)
    md = G.GenericDomain(ctx, space, msh.coords, msh.cp_ids, 1, P.thermal_domain(3, K_COND), [], matrix_free=True)
    md.update_Time()
    md.K_linear_func()
    assert isinstance(md.A, mf.MeshOperator)
    return md


def refusals(mf):
    """{"<entry point>|<kind of handle>": [rc, comparable text ("" when rc == 0)]} on 2 x 2 x 2-element bricks.  Parameters under which each
    physics' own create succeeds: the wrong-physics answers are what is looked at."""
    import torch
    from metafem_jl_amd import _lib

    lib = _lib.lib
    b8, b27 = mf.make_Brick((1.0, 1.0, 1.0), (2, 2, 2), 1, 3), mf.make_Brick((1.0, 1.0, 1.0), (2, 2, 2), 2, 5)
    ctx = b8.ctx
    keep = {"thermal": b8.thermal_operator(K_COND, H, TENV, X0 | X1), "elasticity": b8.elasticity_operator(LAM, MU, TAU, X0 | X1),
            "hex27": b27.thermal_operator_hex27(K_COND, H, TENV, X0 | X1), "elasticity_hex27": b27.elasticity_operator_hex27(LAM, MU, TAU, X0 | X1)}
    md = _mesh_operator(mf, ctx)
    handles = {k: v._h for k, v in keep.items()}
    handles["mesh"] = md.A._h
    out = {}

    def note(entry, kind, rc):
        out[f"{entry}|{kind}"] = [rc, "" if rc == 0 else _message(rc, lib.mfem_last_error().decode())]

    pt = _lib.ThermalParams(K_COND, H, TENV, X0 | X1, 0, 0.0, 0.0)
    pe = _lib.ElasticityParams(LAM, MU, TAU, X0 | X1, 0, (C.c_double * 6)(*([0.0] * 6)))
    sentinel = 123.25
    for kind in KINDS:
        h = handles[kind]
        for entry in CREATES:
            hm = C.c_uint64(1)
            rc = getattr(lib, entry)(ctx._h, h, None, C.byref(hm))
            note(entry, kind, rc)
            assert (hm.value != 0) == (rc == 0)
            if rc == 0:
                _lib.check(lib.mfem_brick_multigrid_destroy(hm))
        note("mfem_brick_operator_set_params", kind, lib.mfem_brick_operator_set_params(h, C.byref(pt)))
        note("mfem_brick_operator_set_elasticity_params", kind, lib.mfem_brick_operator_set_elasticity_params(h, C.byref(pe)))
        xs = torch.full((3 * 125,), 0.5, dtype=torch.float64, device="cuda")
        r = torch.full((3 * 125,), sentinel, dtype=torch.float64, device="cuda")
        rc = lib.mfem_brick_operator_residual_elasticity(ctx._h, h, xs.data_ptr(), r.data_ptr())
        note("mfem_brick_operator_residual_elasticity", kind, rc)
        torch.cuda.synchronize()
        assert bool((r == sentinel).all()) == (rc != 0)  # (a refused call writes nothing)
    return out


def record(mf, directory):
    """writes both files; run on the commit whose answers are to be kept (a job script of the recording session called it there)"""
    os.makedirs(directory, exist_ok=True)
    sha = {"what": "tests/test_gpu_brick_operator_physics.py: digests(mf, case) per case, recorded on the commit before the ops table",
           "cases": {c[0]: digests(mf, c) for c in CASES}}
    with open(os.path.join(directory, os.path.basename(GOLDEN_SHA)), "w") as f:
        json.dump(sha, f, indent=1)
    ref = {"what": "tests/test_gpu_brick_operator_physics.py: refusals(mf), recorded on the commit before the ops table", "answers": refusals(mf)}
    with open(os.path.join(directory, os.path.basename(GOLDEN_REFUSALS)), "w") as f:
        json.dump(ref, f, indent=1)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_physics_keeps_the_parents_bits(mf, case):
    want = json.load(open(GOLDEN_SHA))["cases"][case[0]]
    got = digests(mf, case)
    for key in sorted(set(want) | set(got)):
        print(f"{case[0]} {key}: {got.get(key)} (parent: {want.get(key)})")
    assert got["count_after_one_product"] == 1 and got["count_after_one_apply_dot"] == 1
    assert ("signed_diagonal" in got) == (case[1] in SIGNED) and ("residual" in got) == (case[1] == "elasticity_hex27")
    assert got["cg_jacobi"]["iterations"] >= 1
    assert got == want


def test_refusal_matrix_keeps_the_parents_answers(mf):
    want = json.load(open(GOLDEN_REFUSALS))["answers"]
    assert sorted(want) == sorted(f"{e}|{k}" for k in KINDS for e in CREATES + ["mfem_brick_operator_set_params", "mfem_brick_operator_set_elasticity_params",
                                                                                "mfem_brick_operator_residual_elasticity"])
    got = refusals(mf)
    for key in sorted(want):
        if got[key] != want[key]:
            print(f"{key}: {got[key]} (parent: {want[key]})")
    assert got == want
    # each physics' own entry points serve it
    for kind, create in zip(KINDS[:3], ["mfem_brick_multigrid_create", "mfem_brick_multigrid_create_elasticity", "mfem_brick_multigrid_create_hex27"]):
        assert want[f"{create}|{kind}"][0] == 0
    assert want["mfem_brick_multigrid_create_nonsymmetric|thermal"][0] == 0
    assert want["mfem_brick_operator_residual_elasticity|elasticity_hex27"][0] == 0
    assert all(want[f"{e}|elasticity_hex27"][0] == -3 and "does not exist yet" in want[f"{e}|elasticity_hex27"][1] for e in CREATES)
