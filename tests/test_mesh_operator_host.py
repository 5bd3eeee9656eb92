"""CPU checks of the matrix-free mesh operator: the host decisions of csrc/mesh_operator_decide.h (term compilation, caps, LDS blocks, scratch and
workspace layout, the gate of the solve options), compiled with g++ -- plain, and once more as the same stand-alone program under the address and
undefined-behaviour sanitizers --; every new entry point in the headers, the ctypes table and the Julia binding; and GenericDomain's eligibility
analysis (constant, normal-linear, field-dependent and nonlinear coefficients), which needs no device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mfem_mesh_operator_create", "mfem_mesh_operator_set_elements", "mfem_mesh_operator_add_facets", "mfem_mesh_operator_set_terms",
         "mfem_mesh_operator_destroy", "mfem_mesh_operator_apply", "mfem_mesh_operator_diagonal", "mfem_solve_operator",
         "mfem_debug_mesh_operator_count")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_host_check_mesh_operator(tmp_path, flags):
    exe = str(tmp_path / "host_check_mesh_operator")
    subprocess.run(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "metafem.jl_amd", "csrc"),
                    os.path.join(ROOT, "tools", "host_check_mesh_operator.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip().endswith("OK")


def test_every_operator_entry_point_is_bound_and_declared():
    hdr = open(os.path.join(ROOT, "include", "metafem_mi355x.h")).read() + open(os.path.join(ROOT, "include", "metafem_mi355x_debug.h")).read()
    lib = open(os.path.join(ROOT, "metafem.jl_amd", "_lib.py")).read()
    jl = open(os.path.join(ROOT, "julia", "MI355X.jl")).read()
    for name in NAMES:
        assert f" {name}(" in hdr, name
        assert f'"{name}"' in lib, name
        assert f"(:{name}, lib)" in jl, name
    assert "mfem_operator_term" in hdr and "class OperatorTerm" in lib and "# == mfem_operator_term" in jl


def test_eligibility_analysis(mf):
    """matrix_free_terms / operator_coefficient on the host: what the operator takes and what sends a domain back to the assembled path."""
    from metafem_jl_amd import generic as G, physics as P
    from metafem_jl_amd.affine import operator_coefficient

    k = 0.6
    # constant coefficients: the thermal, elasticity, inertia and penalty forms
    parts, reason = G.matrix_free_terms(P.thermal_domain(3, k, alpha=0.7, Tenv=300.0, C=4.0), [P.thermal_convection(25.0, 293.15)])
    assert reason is None and len(parts) == 2
    assert sorted(c.c0 for _, c in parts[0]) == sorted([-4.0, -k, -k, -k, -0.7]) and all(c.normal == (0.0, 0.0, 0.0) for _, c in parts[0])
    assert [(g.dual_s, g.base_s, c.c0) for g, c in parts[1]] == [(0, 0, -25.0)]
    parts, reason = G.matrix_free_terms(P.merge(P.elasticity_domain(3, 1.7, 0.6), P.elasticity_inertia(3, 7.8, c=0.3)), [P.penalty([0, 1, 2], 37.0)])
    assert reason is None and len(parts[0]) >= 21 + 3
    # normal-linear on facets: the Nitsche wall k n_d T_d
    wall = P.thermal_fixed(2, 1000.0, 1173.15, k)
    parts, reason = G.matrix_free_terms(P.thermal_domain(2, k), [wall])
    assert reason is None
    got = {(g.base_s): (c.c0, c.normal) for g, c in parts[1]}
    assert got == {0: (-1000.0, (0.0, 0.0, 0.0)), 1: (0.0, (k, 0.0, 0.0)), 2: (0.0, (0.0, k, 0.0))}
    # ... but not on elements, where no normal exists
    parts, reason = G.matrix_free_terms(wall, [])
    assert parts is None and "domain" in reason
    mixed = G.WeakForm(normals=[("n0", 0), ("n1", 1)])
    mixed.linear_gradients.append(G.GradTerm(0, 0, 0, 1, lambda env: 2.0 - 3.0 * env["n1"] + 0.5 * env["dt"]))
    c = operator_coefficient(mixed.linear_gradients[0], mixed, facet=True, t=0.0, dt=0.25)
    assert c is not None and c.c0 == 2.125 and c.normal == (0.0, -3.0, 0.0)
    assert operator_coefficient(mixed.linear_gradients[0], mixed, facet=False) is None
    # field-dependent, external-dependent and nonlinear-in-the-normal coefficients
    for fn in (lambda env: -k * env["T"], lambda env: env["s"], lambda env: env["n0"] * env["n1"], lambda env: env["n0"] ** 2,
               lambda env: abs(env["n0"]), lambda env: 1.0 if env["n0"] > 0 else 2.0):
        wf = G.WeakForm(inner_vars=[("T", 0, 0, 0)], cp_ext_vars=[("s", "s", 0)], normals=[("n0", 0), ("n1", 1)])
        wf.linear_gradients.append(G.GradTerm(0, 0, 0, 0, fn))
        assert operator_coefficient(wf.linear_gradients[0], wf, facet=True) is None
        parts, reason = G.matrix_free_terms(G.WeakForm(), [wf])
        assert parts is None and "boundary group 0" in reason
    # a nonlinear gradient anywhere
    parts, reason = G.matrix_free_terms(P.thermal_domain(3, k), [P.thermal_convection(25.0, 293.15, em=0.8, sigma_b=5.67e-8)])
    assert parts is None and "nonlinear" in reason
