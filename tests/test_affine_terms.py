"""Affine analysis of residual terms (metafem.jl_amd/affine.py) and their packing into the ABI structs of the fused mesh residual (CPU)."""
import ctypes as C

import numpy as np
import pytest
import torch


def _forms(physics):
    return {
        "thermal_domain": physics.thermal_domain(3, 0.7, alpha=2.5, Tenv=300.0, C=4.0),
        "thermal_domain_2d": physics.thermal_domain(2, 1.3),
        "thermal_convection": physics.thermal_convection(25.0, 293.15),
        "thermal_fixed_2d": physics.thermal_fixed(2, 1000.0, 1173.15, 0.6),
        "thermal_fixed_3d": physics.thermal_fixed(3, 1000.0, 1173.15, 0.6),
        "elasticity_2d": physics.elasticity_domain(2, 1.2e3, 0.8e3),
        "elasticity_3d": physics.elasticity_domain(3, 1.2e3, 0.8e3),
        "inertia": physics.elasticity_inertia(3, 7.8, c=0.3),
        "inertia_undamped": physics.elasticity_inertia(2, 7.8),
        "penalty": physics.penalty([0, 2], 1e6),
        "penalty_wall": physics.penalty([0, 1, 2], 1e6, wall_syms=["w0", "w1", "w2"]),
        "traction_3d": physics.traction(3, "sl"),
        "traction_2d_row": physics.traction(2, "sg", rows=[1]),
    }


def _random_env(wf, g, shape=(6, 9), t=0.25, dt=0.5):
    env, val = {}, {}
    for name, pos, s, td in wf.inner_vars:
        env[name] = torch.randn(shape, generator=g, dtype=torch.float64)
        val[("x", pos, td, s)] = env[name]
    for name, sym, s in wf.cp_ext_vars:
        env[name] = torch.randn(shape, generator=g, dtype=torch.float64)
        val[("ext", sym, s)] = env[name]
    for name, comp in wf.normals:
        env[name] = torch.randn(shape, generator=g, dtype=torch.float64)
        val[("n", comp)] = env[name]
    env["t"], env["dt"] = t, dt
    return env, val


def _reconstruct(d, val, shape):
    r = torch.full(shape, d.c0, dtype=torch.float64)
    for s, n, c in d.pairs:
        p = torch.full(shape, c, dtype=torch.float64)
        if n is not None:
            p = p * val[("n", n)]
        if s is not None:
            p = p * val[s]
        r = r + p
    return r


@pytest.mark.parametrize("form", [
    "thermal_domain", "thermal_domain_2d", "thermal_convection", "thermal_fixed_2d", "thermal_fixed_3d", "elasticity_2d", "elasticity_3d",
    "inertia", "inertia_undamped", "penalty", "penalty_wall", "traction_3d", "traction_2d_row"])
def test_every_linear_example_residual_is_affine(mf, form):
    from metafem_jl_amd import physics
    from metafem_jl_amd.generic import affine_residual

    wf = _forms(physics)[form]
    assert wf.residues
    g = torch.Generator().manual_seed(7)
    for term in wf.residues:
        d = affine_residual(term, wf, t=0.25, dt=0.5)
        assert d is not None, (form, term)
        assert (d.dual_pos, d.dual_s) == (term.dual_pos, term.dual_s)
        for _ in range(3):
            env, val = _random_env(wf, g)
            got = term.fn(env)
            if not torch.is_tensor(got):
                got = torch.full((6, 9), float(got), dtype=torch.float64)
            ref = _reconstruct(d, val, (6, 9))
            assert (got - ref).abs().max() <= 1e-14 * max(1.0, float(got.abs().max()))


def test_descriptions_carry_the_expected_coefficients(mf):
    from metafem_jl_amd import physics
    from metafem_jl_amd.generic import affine_residual

    wf = physics.thermal_fixed(3, 1000.0, 1173.15, 0.6)
    d = affine_residual(wf.residues[0], wf)
    assert d.c0 == pytest.approx(1000.0 * 1173.15)
    pairs = {(s, n): c for s, n, c in d.pairs}
    assert pairs[(("x", 0, 0, 0), None)] == -1000.0
    for j in range(3):
        assert pairs[(("x", 0, 0, 1 + j), j)] == pytest.approx(0.6)
    wf = physics.traction(3, "sl", rows=[0])
    d = affine_residual(wf.residues[0], wf)
    assert d.c0 == 0.0 and {(s, n) for s, n, _ in d.pairs} == {(("ext", "sl1", 0), 0), (("ext", "sl6", 0), 1), (("ext", "sl5", 0), 2)}
    wf = physics.elasticity_inertia(3, 7.8, c=0.3)
    d = affine_residual(wf.residues[1], wf)
    assert {s: c for s, _, c in d.pairs} == {("x", 1, 1, 0): pytest.approx(-7.8 * 0.3), ("x", 1, 2, 0): pytest.approx(-7.8)}


def test_time_enters_as_a_plain_float(mf):
    from metafem_jl_amd.generic import ResTerm, WeakForm, affine_residual

    wf = WeakForm(inner_vars=[("T", 0, 0, 0)])
    term = ResTerm(0, 0, lambda env: np.sin(env["t"]) * env["T"] + env["dt"] if env["t"] > 1.0 else env["T"])
    d = affine_residual(term, wf, t=2.0, dt=0.1)
    assert d.c0 == pytest.approx(0.1) and d.pairs == [(("x", 0, 0, 0), None, pytest.approx(np.sin(2.0)))]
    assert affine_residual(term, wf, t=0.5, dt=0.1).pairs == [(("x", 0, 0, 0), None, 1.0)]


def test_non_affine_terms_are_refused(mf):
    from metafem_jl_amd import physics
    from metafem_jl_amd.generic import ResTerm, WeakForm, affine_residual

    rad = physics.thermal_convection(25.0, 293.15, em=0.8, sigma_b=5.67e-8)
    assert affine_residual(rad.residues[0], rad) is not None
    assert affine_residual(rad.residues[1], rad) is None  # T^4
    wf = WeakForm(inner_vars=[("T", 0, 0, 0), ("T_0", 0, 1, 0), ("u", 1, 0, 0)])
    refused = [
        lambda env: torch.exp(env["T"]),
        lambda env: env["T"] * env["u"],
        lambda env: env["T"] if env["T"] > 0 else 0.0,
        lambda env: torch.where(env["T"] > 0, env["T"], 0.0),
        lambda env: env["T_0"] ** 2,
        lambda env: 1.0 / env["T"],
        lambda env: abs(env["T"]),
        lambda env: env["missing"],
    ]
    for fn in refused:
        assert affine_residual(ResTerm(0, 0, fn), wf) is None
    assert affine_residual(ResTerm(0, 0, lambda env: 3.0 * (env["T"] - 2.0 * env["u"]) / 4.0 + env["T_0"] ** 1), wf) is not None


def test_the_numerical_check_rejects_a_probe_mismatch(mf):
    """A term that answers the probes differently from tensors (here: it inspects the type) fails the check."""
    from metafem_jl_amd.generic import ResTerm, WeakForm, affine_residual

    wf = WeakForm(inner_vars=[("T", 0, 0, 0)])
    sneaky = ResTerm(0, 0, lambda env: env["T"] if not torch.is_tensor(env["T"]) else env["T"] * env["T"])
    assert affine_residual(sneaky, wf, check=False) is not None
    assert affine_residual(sneaky, wf) is None


def test_packing_deduplicates_symbols_and_fills_the_structs(mf):
    from metafem_jl_amd import _lib, physics
    from metafem_jl_amd.affine import pack_affine
    from metafem_jl_amd.generic import affine_residual

    wf = physics.elasticity_domain(3, 1.2e3, 0.8e3)
    descs = [affine_residual(t, wf) for t in wf.residues]
    seen = []

    def source(k):
        seen.append(k)
        _, pos, td, word = k
        return word, 1000 * pos + 7 * td, 0x1000

    syms, nsym, terms, nterm, keys = pack_affine(descs, source)
    assert nsym == 9 and nterm == 9 and len(set(keys)) == 9 and sorted(seen) == sorted(keys)
    assert C.sizeof(_lib.AffineTerm) == 4 * 4 + 8 + 8 * 4 * 2 + 8 * 8 and C.sizeof(_lib.ResSymbol) == 24
    for i, d in enumerate(descs):
        t = terms[i]
        assert (t.dual_pos, t.dual_sd, t.n_pairs) == (d.dual_pos, d.dual_s, len(d.pairs))
        for p, (s, n, c) in enumerate(d.pairs):
            assert keys[t.sym[p]] == s and t.normal[p] == -1 and t.coef[p] == c
            assert syms[t.sym[p]].word == s[3] and syms[t.sym[p]].shift == 1000 * s[1]
    # facets: a constant times a normal is a pair without symbol
    wf = physics.traction(2, "sg")
    syms, nsym, terms, nterm, keys = pack_affine([affine_residual(t, wf) for t in wf.residues], lambda k: (k[2], 0, 0x2000))
    assert nsym == 3 and all(k[0] == "ext" for k in keys)


def test_packing_caps_raise(mf):
    from metafem_jl_amd.affine import AffineResidual, CapsExceeded, pack_affine

    src = lambda k: (0, 0, 0x1000)
    many_syms = [AffineResidual(0, 0, 0.0, [(("x", i, 0, 0), None, 1.0)]) for i in range(17)]
    with pytest.raises(CapsExceeded):
        pack_affine(many_syms, src)
    pack_affine(many_syms[:16], src)
    with pytest.raises(CapsExceeded):
        pack_affine([AffineResidual(0, 0, 1.0, [])] * 49, src)
    with pytest.raises(CapsExceeded):
        pack_affine([AffineResidual(0, 0, 0.0, [(("x", i, 0, 0), None, 1.0) for i in range(9)])], src)
    pack_affine([AffineResidual(0, 0, 0.0, [(("x", i, 0, 0), None, 1.0) for i in range(8)])], src)
