"""Affine analysis of residual terms for the fused mesh residual (mfem_mesh_residual_elements / _facets).

A residual term `ResTerm(dual_pos, dual_s, fn)` is affine when fn(env) is, at every Gauss point,
    c0 + sum_p coef_p [n_j] u_p
with u_p an inner variable (a word of x_star) or a nodal external, and n_j an optional component of the outward normal (facets).
`affine_residual` finds that description by evaluating fn once on probe objects that carry such sums and refuse everything else
(a product of two fields, a power other than 0 or 1, a torch / numpy function, a comparison or a branch on a value), then checks
it once numerically against fn on random tensors.  This generalises `generic.constant_coefficient` (the case without symbols).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib

SymKey = Tuple  # ("x", field position, time level, word) | ("ext", controlpoint symbol, word)


class _NotAffine(Exception):
    pass


class _Aff:
    """sum over monomials (symbol or None, normal component or None) -> coefficient."""

    __array_ufunc__ = None  # (numpy scalars defer to the reflected operators below)
    __slots__ = ("m",)

    def __init__(self, m: Dict[Tuple, float]):
        self.m = m

    @staticmethod
    def _lift(v) -> "_Aff":
        if isinstance(v, _Aff):
            return v
        if isinstance(v, (bool, int, float)) or (hasattr(v, "dtype") and getattr(v, "shape", None) == () and not torch.is_tensor(v)):
            return _Aff({(None, None): float(v)})
        raise _NotAffine(type(v).__name__)

    def __add__(self, o):
        o = _Aff._lift(o)
        m = dict(self.m)
        for k, c in o.m.items():
            m[k] = m.get(k, 0.0) + c
        return _Aff(m)

    __radd__ = __add__

    def __neg__(self):
        return _Aff({k: -c for k, c in self.m.items()})

    def __pos__(self):
        return self

    def __sub__(self, o):
        return self + (-_Aff._lift(o))

    def __rsub__(self, o):
        return _Aff._lift(o) + (-self)

    def __mul__(self, o):
        o = _Aff._lift(o)
        m: Dict[Tuple, float] = {}
        for (s1, n1), c1 in self.m.items():
            for (s2, n2), c2 in o.m.items():
                if (s1 is not None and s2 is not None) or (n1 is not None and n2 is not None):
                    raise _NotAffine("product of two fields or two normals")
                k = (s1 if s1 is not None else s2, n1 if n1 is not None else n2)
                m[k] = m.get(k, 0.0) + c1 * c2
        return _Aff(m)

    __rmul__ = __mul__

    def __truediv__(self, o):
        if isinstance(o, _Aff):
            if set(o.m) != {(None, None)}:
                raise _NotAffine("division by a field")
            o = o.m[(None, None)]
        return self * (1.0 / float(o))

    def __pow__(self, e):
        if isinstance(e, (int, float)) and float(e) in (0.0, 1.0):
            return _Aff({(None, None): 1.0}) if e == 0 else self
        raise _NotAffine("power of a field")

    def _refuse(self, *a, **k):
        raise _NotAffine("a value is inspected")

    __rtruediv__ = __rpow__ = __lt__ = __le__ = __gt__ = __ge__ = __eq__ = __ne__ = _refuse
    __bool__ = __float__ = __int__ = __index__ = __abs__ = __round__ = _refuse
    __hash__ = None


class _ProbeEnv(dict):
    """Inner variables, externals and normals as probes; t / dt plain floats; anything else raises."""

    def __missing__(self, key):
        raise _NotAffine(f"unknown name {key!r}")


@dataclass
class AffineResidual:
    """dual word (dual_pos, dual_s) x (c0 + sum_p coef_p [n_normal_p] symbol_p); symbol None = the constant 1."""
    dual_pos: int
    dual_s: int
    c0: float
    pairs: List[Tuple[Optional[SymKey], Optional[int], float]]

    def symbols(self) -> List[SymKey]:
        out: List[SymKey] = []
        for s, _, _ in self.pairs:
            if s is not None and s not in out:
                out.append(s)
        return out


def _names(wf) -> Dict[str, object]:
    """name -> what it stands for: a SymKey, or ("n", component)."""
    out: Dict[str, object] = {}
    for name, pos, s, td in wf.inner_vars:
        out[name] = ("x", pos, td, s)
    for name, sym, s in wf.cp_ext_vars:
        out[name] = ("ext", sym, s)
    for name, comp in wf.normals:
        out[name] = ("n", comp)
    return out


def affine_residual(term, wf, t: float = 0.0, dt: float = 1.0, check: bool = True) -> Optional[AffineResidual]:
    """The affine description of `term` (a ResTerm of `wf`), or None if fn is not affine in the fields / externals (with normals
    as factors).  env["t"], env["dt"] are the plain floats t, dt.  check: compare the description once with fn on random tensors."""
    names = _names(wf)
    env = _ProbeEnv()
    for name, what in names.items():
        env[name] = _Aff({(None, what[1]): 1.0}) if what[0] == "n" else _Aff({(what, None): 1.0})
    env["t"], env["dt"] = float(t), float(dt)
    try:
        v = term.fn(env)
        v = _Aff._lift(v)
    except Exception:
        return None
    c0 = v.m.get((None, None), 0.0)
    pairs = [(s, n, c) for (s, n), c in v.m.items() if (s, n) != (None, None) and c != 0.0]
    if not all(math.isfinite(c) for c in [c0] + [c for _, _, c in pairs]):
        return None
    desc = AffineResidual(term.dual_pos, term.dual_s, float(c0), pairs)
    if check and not _check(term, desc, names, t, dt):
        return None
    return desc


def _check(term, desc: AffineResidual, names, t, dt, shape=(5, 7)) -> bool:
    g = torch.Generator().manual_seed(0xAFF1)
    env: Dict[str, object] = {}
    val: Dict[object, torch.Tensor] = {}
    for name, what in names.items():
        x = torch.rand(shape, generator=g, dtype=torch.float64) * 2.0 - 1.0
        env[name] = x
        val[what if what[0] != "n" else ("n", what[1])] = x
    env["t"], env["dt"] = float(t), float(dt)
    try:
        got = term.fn(env)
    except Exception:
        return False
    ref = torch.full(shape, desc.c0, dtype=torch.float64)
    scale = torch.full(shape, abs(desc.c0), dtype=torch.float64)
    for s, n, c in desc.pairs:
        p = torch.full(shape, c, dtype=torch.float64)
        if n is not None:
            p = p * val[("n", n)]
        if s is not None:
            p = p * val[s]
        ref = ref + p
        scale = scale + p.abs()
    if not torch.is_tensor(got):
        try:
            got = torch.full(shape, float(got), dtype=torch.float64)
        except Exception:
            return False
    if got.shape != ref.shape:
        return False
    return bool(((got.to(torch.float64) - ref).abs() <= 1e-13 * (scale + 1e-300)).all())


@dataclass
class OperatorCoefficient:
    """The coefficient of a linear gradient term the matrix-free operator takes: c0 + sum_j normal[j] n_j."""
    c0: float
    normal: Tuple[float, float, float]


def operator_coefficient(term, wf, facet: bool, t: float = 0.0, dt: float = 1.0, check: bool = True) -> Optional[OperatorCoefficient]:
    """The constant (on facets: constant plus normal-linear) description of the coefficient of `term` (a GradTerm of `wf`), or None if fn reads a
    field or an external, is not linear in the normal components, or -- on elements -- reads a normal at all.  The probes are those of
    `affine_residual`: only the normals, t and dt exist in the probe environment.  check: compare once with fn on random normals."""
    comps = {name: comp for name, comp in wf.normals}
    env = _ProbeEnv()
    for name, comp in comps.items():
        env[name] = _Aff({(None, comp): 1.0})
    env["t"], env["dt"] = float(t), float(dt)
    try:
        v = _Aff._lift(term.fn(env))
    except Exception:
        return None
    nrm = [0.0, 0.0, 0.0]
    for (s, n), c in v.m.items():
        if s is not None or (n is not None and not 0 <= n < 3):
            return None
        if n is not None:
            nrm[n] += c
    c0 = float(v.m.get((None, None), 0.0))
    if not all(math.isfinite(c) for c in [c0] + nrm):
        return None
    if not facet and any(c != 0.0 for c in nrm):
        return None
    if check:
        g = torch.Generator().manual_seed(0x0FE2)
        shape = (5, 7)
        vals = {name: torch.rand(shape, generator=g, dtype=torch.float64) * 2.0 - 1.0 for name in comps}
        num: Dict[str, object] = dict(vals)
        num["t"], num["dt"] = float(t), float(dt)
        try:
            got = term.fn(num)
            if not torch.is_tensor(got):
                got = torch.full(shape, float(got), dtype=torch.float64)
        except Exception:
            return None
        ref = torch.full(shape, c0, dtype=torch.float64)
        scale = torch.full(shape, abs(c0), dtype=torch.float64)
        for name, comp in comps.items():
            ref = ref + nrm[comp] * vals[name]
            scale = scale + abs(nrm[comp]) * vals[name].abs()
        if got.shape != ref.shape or not bool(((got.to(torch.float64) - ref).abs() <= 1e-13 * (scale + 1e-300)).all()):
            return None
    return OperatorCoefficient(c0, (nrm[0], nrm[1], nrm[2]))


class CapsExceeded(ValueError):
    """The terms of one launch exceed MFEM_RES_MAX_SYMBOLS / _TERMS / _PAIRS: they take the operator path."""


def pack_affine(descs: Sequence[AffineResidual], source: Callable[[SymKey], Tuple[int, int, int]]):
    """ABI structs of one fused residual launch.  source(symbol) -> (word, shift, device pointer).  Symbols are deduplicated over
    the terms.  Returns (symbols array, n_symbols, terms array, n_terms, symbol keys in array order); raises CapsExceeded."""
    keys: List[SymKey] = []
    for d in descs:
        for s in d.symbols():
            if s not in keys:
                keys.append(s)
    if len(keys) > _lib.MAX_RES_SYMBOLS:
        raise CapsExceeded(f"{len(keys)} symbols > {_lib.MAX_RES_SYMBOLS}")
    if len(descs) > _lib.MAX_RES_TERMS:
        raise CapsExceeded(f"{len(descs)} terms > {_lib.MAX_RES_TERMS}")
    syms = (_lib.ResSymbol * max(len(keys), 1))()
    for i, k in enumerate(keys):
        word, shift, ptr = source(k)
        syms[i] = _lib.ResSymbol(word, 0, shift, ptr)
    terms = (_lib.AffineTerm * max(len(descs), 1))()
    for i, d in enumerate(descs):
        if len(d.pairs) > _lib.MAX_RES_PAIRS:
            raise CapsExceeded(f"a term of {len(d.pairs)} pairs > {_lib.MAX_RES_PAIRS}")
        t = terms[i]
        t.dual_pos, t.dual_sd, t.n_pairs, t.c0 = d.dual_pos, d.dual_s, len(d.pairs), d.c0
        for p, (s, n, c) in enumerate(d.pairs):
            t.sym[p] = -1 if s is None else keys.index(s)
            t.normal[p] = -1 if n is None else n
            t.coef[p] = c
    return syms, len(keys), terms, len(descs), keys
