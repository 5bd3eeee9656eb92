"""CPU checks of the variable terms of the matrix-free mesh operator: the host decisions of csrc/mesh_operator_decide.h for mixed constant and
variable term lists (tools/host_check_mesh_operator_var.cpp), compiled with g++ -- plain, and once more as the same stand-alone program under the
address and undefined-behaviour sanitizers --; the new entry point in the header, the ctypes table and the Julia binding (with the static checks
of tests/test_julia_binding.py on its ccall); and the classifier of GenericDomain(matrix_free="any"), which needs no device."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mfem_mesh_operator_set_variable_terms"


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_host_check_mesh_operator_var(tmp_path, flags):
    exe = str(tmp_path / "host_check_mesh_operator_var")
    subprocess.run(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "metafem.jl_amd", "csrc"),
                    os.path.join(ROOT, "tools", "host_check_mesh_operator_var.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip().endswith("OK")


def test_the_entry_point_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read()
    lib = open(os.path.join(ROOT, "metafem.jl_amd", "_lib.py")).read()
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"int {NAME}(uint64_t op, int32_t part, int32_t n_terms, const mfem_kval_term* terms, const double* vals);" in hdr
    assert f'"{NAME}": (c_int, [c_uint64, c_int32, c_int32, C.POINTER(KvalTerm), P])' in lib
    assert f"(:{NAME}, lib)" in jl
    assert NAME in integ and "operator_variable_terms!" in integ
    head = [ln for ln in hdr.splitlines() if ln.startswith("/* ---- matrix-free operator on unstructured meshes")]
    assert len(head) == 1 and "variable terms" in head[0]  # (the section's header comment no longer says constant-coefficient terms only)
    src = open(os.path.join(ROOT, "metafem.jl_amd", "csrc", "mesh_operator.hip")).read()
    assert f'extern "C" int {NAME}(' in src


def test_the_julia_ccall_matches_the_header():
    """Argument count and the Julia type of every C parameter (tests/test_julia_binding.py walks this ccall too, with every other one)."""
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    m = re.search(r"ccall\(\(:" + NAME + r", lib\), Cint,\s*\(([^)]*)\)", jl)
    assert m, "ccall not found"
    types = [t.strip() for t in m.group(1).split(",") if t.strip()]
    assert types == ["UInt64", "Int32", "Int32", "Ptr{KvalTerm}", "Ptr{Cvoid}"]


def test_classifier(mf):
    """matrix_free_parts: the constant terms as matrix_free_terms takes them; every nonlinear gradient and every linear gradient with a field-,
    external- or nonlinearly normal-dependent coefficient variable; matrix_free_terms keeps its answers."""
    from metafem_jl_amd import generic as G, physics as P

    k = 0.6
    # constant forms: the same terms as matrix_free_terms, nothing variable
    forms = (P.thermal_domain(3, k, alpha=0.7, Tenv=300.0, C=4.0), [P.thermal_convection(25.0, 293.15)])
    parts = G.matrix_free_parts(*forms)
    ref, reason = G.matrix_free_terms(*forms)
    assert reason is None and len(parts) == 2
    for p, r in zip(parts, ref):
        assert [(g, c.c0, c.normal) for g, c in p.constant] == [(g, c.c0, c.normal) for g, c in r]
        assert p.variable == [] and p.nonlinear == [] and p.variable_linear == []
    # radiation on the facets: the constant -h stays constant, the radiative gradient is the one variable term
    rad = P.thermal_convection(25.0, 293.15, em=0.8, sigma_b=5.67e-8)
    parts = G.matrix_free_parts(P.thermal_domain(3, k), [rad])
    assert len(parts[0].constant) == 3 and parts[0].variable == []
    assert [(g.dual_s, g.base_s, c.c0) for g, c in parts[1].constant] == [(0, 0, -25.0)]
    assert parts[1].variable == rad.nonlinear_gradients and parts[1].variable_linear == []
    assert G.matrix_free_terms(P.thermal_domain(3, k), [rad])[0] is None  # (the opt-in boundary: matrix_free=True still refuses)
    # the Nitsche wall: normal-linear coefficients are constant terms on facets, variable on elements (no normal there)
    wall = P.thermal_fixed(2, 1000.0, 1173.15, k)
    parts = G.matrix_free_parts(P.thermal_domain(2, k), [wall])
    assert len(parts[1].constant) == 3 and parts[1].variable == []
    parts = G.matrix_free_parts(wall, [])
    assert len(parts[0].constant) == 1 and len(parts[0].variable_linear) == 2 and parts[0].nonlinear == []
    # field-, external- and nonlinearly normal-dependent linear gradients; slot order: the linear ones, then the nonlinear ones
    wf = G.WeakForm(inner_vars=[("T", 0, 0, 0)], cp_ext_vars=[("s", "s", 0)], normals=[("n0", 0), ("n1", 1)])
    fns = (lambda env: -k * env["T"], lambda env: env["s"], lambda env: env["n0"] * env["n1"], lambda env: abs(env["n0"]))
    for fn in fns:
        wf.linear_gradients.append(G.GradTerm(0, 0, 0, 0, fn))
    wf.linear_gradients.append(G.GradTerm(0, 0, 0, 1, lambda env: 2.0 - 3.0 * env["n1"] + 0.5 * env["dt"]))
    wf.nonlinear_gradients.append(G.GradTerm(0, 1, 0, 0, lambda env: env["T"] ** 2))
    part = G.matrix_free_parts(G.WeakForm(), [wf], t=0.0, dt=0.25)[1]
    assert [g.fn for g in part.variable_linear] == list(fns)
    assert [(c.c0, c.normal) for _, c in part.constant] == [(2.125, (0.0, -3.0, 0.0))]
    assert part.variable == part.variable_linear + wf.nonlinear_gradients and len(part.variable) == 5
    # Neo-Hookean: 81 nonlinear gradients on the elements, the penalty wall constant
    from oracle import hyperelastic as he

    hw = he.domain_weakform(dict(mu=1.0, lam=1.5), "neo_hookean")
    parts = G.matrix_free_parts(hw, [P.penalty([0, 1, 2], 37.0)])
    assert parts[0].constant == [] and len(parts[0].variable) == 81 and len(parts[1].constant) == 3 and parts[1].variable == []
