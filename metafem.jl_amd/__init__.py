"""metafem.jl_amd -- host-side mirror of MetaFEM.jl's assembly-and-solve interface over the
MI355X C ABI (libmetafem_mi355x.so).

The reference's host language is Julia, which this image does not have; the
Julia `ccall` shim a maintainer would add is in INTEGRATION.md.  This Python layer is the
runnable stand-in: same entry points, argument meaning and error behaviour as the reference
functions it names, with torch used only for device memory and streams.

  FEM_SpMat_CSR / mul_            src/misc/04_GPU_Utils.jl:120,131
  iterative_Solve                 src/solver/linear_solver/02_Preconditioner.jl:32-76
  Pr_Jacobi_ kernels              :103-148
  make_Brick + mesh_Classical     src/mesh/ref_geometry/201_Helper_TM.jl:36-51; unstructured_mesh/2_Interface.jl:7
  assemble_Global_Variables       src/solver/03_GlobalAssembly.jl:6-37
  update_OneStep                  src/solver/04_Time_Domain.jl:59-80

There is no CPU fallback: importing this package without the built HIP library raises, and
every call goes through the C ABI.
"""
from __future__ import annotations

import ctypes as C
import weakref
import math
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import torch

from . import _lib
from ._lib import (ElasticityParams, MetaFEMError, OpLayout, SolveOptions, SolveStats, ThermalParams, check, lib)

__all__ = ["Context", "FEM_SpMat_CSR", "MeshOperator", "BrickOperator", "BrickMultigrid", "MultigridRefused", "Pr_Multigrid_", "multigrid_plan", "multigrid_plan_hex27", "ElasticityBrickOperator", "Hex27BrickOperator", "BrickOperatorRefused", "brick_operator_refusal",
           "brick_operator_hex27_refusal", "Hex27ElasticityBrickOperator", "brick_operator_elasticity_hex27_refusal", "mul_", "tmul_", "dot", "nrm2", "axpby_", "FEM_rand", "normalized_norm",
           "iterative_Solve", "Brick", "make_Brick", "ThermalDomain", "ElasticityDomain", "MetaFEMError", "SolveStats",
           "cg_", "bicgstabl_GS_", "idrs_", "cgs2_", "gmres_", "cgs_", "tfqmr_", "lsqr_", "FACE_BITS"]

# solver / preconditioner selectors (the reference passes Julia functions: Sv_func! = idrs! ...)
cg_, bicgstabl_GS_, idrs_, cgs2_, gmres_, cgs_, tfqmr_, lsqr_ = 0, 1, 2, 3, 4, 5, 6, 7
Identity, Pr_Jacobi_, Pr_Jacobi_colnorm_ = 0, 1, 2
Pr_Multigrid_ = 3  # a geometric multigrid V-cycle: cg_ on a hex-8 thermal BrickOperator (BrickOperator.multigrid), or on an ElasticityBrickOperator
# or a Hex27BrickOperator to which its multigrid() has attached a hierarchy (no default one is made for those two)
Pl_Jacobi_, Pl_Jacobi_rownorm_ = 1, 2  # Pl_func selectors (02_Preconditioner.jl:155-168)

# reference local face ids (ref_geometry/002_Initialization.jl:8): 1 z=0, 2 y=0, 3 x=L, 4 y=L, 5 x=0, 6 z=L
FACE_BITS = {"z0": 1 << 0, "y0": 1 << 1, "x1": 1 << 2, "y1": 1 << 3, "x0": 1 << 4, "z1": 1 << 5}
ALL_FACES = 0x3F


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _need(t: torch.Tensor, dtype, name: str, n: Optional[int] = None) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise MetaFEMError(f"{name} must be a device (cuda) torch tensor")
    if t.dtype != dtype:
        raise MetaFEMError(f"{name} must have dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise MetaFEMError(f"{name} must be contiguous")
    if n is not None and t.numel() < n:
        raise MetaFEMError(f"{name} has {t.numel()} elements, needs {n}")


class Context:
    """One device + stream binding.  Uses torch's current stream so kernels order with torch ops."""

    def __init__(self, device: int = 0):
        if not torch.cuda.is_available():
            raise MetaFEMError("no HIP device visible: the MI355X backend has no CPU fallback")
        self.device = device
        torch.cuda.set_device(device)
        self._h = C.c_void_p()
        # handles created on this context (patterns, bricks, communicators): closed before the context itself, whatever the order in
        # which the interpreter drops the Python objects (a pattern destroyed after its context would touch freed memory)
        self._children = weakref.WeakSet()
        stream = torch.cuda.current_stream(device).cuda_stream
        check(lib.mfem_context_create(device, C.c_void_p(stream), C.byref(self._h)))

    def use_current_stream(self):
        check(lib.mfem_context_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def sync(self):
        check(lib.mfem_context_sync(self._h))

    def close(self):
        if self._h:
            for child in list(self._children):
                try:
                    child.close()
                except Exception:
                    pass
            lib.mfem_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx: Optional[Context] = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(torch.cuda.current_device())
    return _default_ctx


class FEM_SpMat_CSR:
    """CSR pattern handle: FEM_SpMat_CSR(K_J_ptr, K_J, K_vals, dims) (04_GPU_Utils.jl:120) without the
    values (they change every Newton step; pass them per call).  `rowptr` / `colidx` are BORROWED by the library and FROZEN for
    the lifetime of the handle: it keeps what it learnt from them at creation (row blocks, tiles that repeat one column-offset
    list, later the solver layouts).  After rewriting them in place call `replan()`; a different pattern needs a new handle."""

    def __init__(self, rowptr: torch.Tensor, colidx: torch.Tensor, n: int, index_base: int = 0,
                 ctx: Optional[Context] = None, _handle=None):
        self.ctx = ctx or default_context()
        self.rowptr, self.colidx = rowptr, colidx  # keep alive: the library borrows them
        self._owned = _handle is not None
        if _handle is not None:
            self._h = _handle
        else:
            if rowptr.dtype not in (torch.int32, torch.int64):
                raise MetaFEMError("rowptr must be int32 or int64")
            _need(rowptr, rowptr.dtype, "rowptr", n + 1)
            _need(colidx, torch.int32, "colidx")
            self._h = C.c_void_p()
            check(lib.mfem_csr_create(self.ctx._h, n, colidx.numel(), _ptr(rowptr), 64 if rowptr.dtype == torch.int64 else 32,
                                      _ptr(colidx), index_base, C.byref(self._h)))
        self.n = int(lib.mfem_csr_n(self._h))
        self.nnz = int(lib.mfem_csr_nnz(self._h))
        self.index_base = index_base
        self.ctx._children.add(self)

    @property
    def ncols(self) -> int:
        """Columns the pattern addresses = length of x and of a per-column vector (n + ghost entries for a slab pattern)."""
        return int(lib.mfem_csr_ncols(self._h))

    def replan(self):
        """Re-inspect the (rewritten in place) pattern arrays: mfem_csr_replan."""
        check(lib.mfem_csr_replan(self.ctx._h, self._h))

    def spmv_bytes(self):
        """(bytes one mul_ launch moves by design, column entries it reads): mfem_csr_spmv_bytes."""
        b, c = C.c_int64(), C.c_int64()
        check(lib.mfem_csr_spmv_bytes(self.ctx._h, self._h, C.byref(b), C.byref(c)))
        return b.value, c.value

    def close(self):
        if self._h:
            lib.mfem_csr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MeshOperator:
    """Matrix-free K of an unstructured mesh (mfem_mesh_operator_*, csrc/mesh_operator.hip): stands where a FEM_SpMat_CSR and its values stand --
    `mul_(b, A, None, x)` and `iterative_Solve(A, None, residue, ...)` take it -- and holds no matrix: the mesh arrays (borrowed: coords SoA
    [dim * ncp], controlpoint_IDs (nel, itp) C order), the reference tables and the adjacency of each part, and the terms
    `(dual_sd, base_sd, block, coef[, (n0, n1, n2)])` of the elements and of every facet group."""

    def __init__(self, ctx: "Context", dim: int, itp: int, nel: int, ncp: int, n_fields: int, coords: torch.Tensor, controlpoint_IDs: torch.Tensor,
                 index_base: int = 1):
        self.ctx = ctx
        _need(coords, torch.float64, "coords", dim * ncp)
        _need(controlpoint_IDs, torch.int32, "controlpoint_IDs", nel * itp)
        self._keep = [coords, controlpoint_IDs]  # the library borrows every array
        self._var_keep = {}  # part -> the coefficient array of its variable terms
        self.n_fields, self.ncp = n_fields, ncp
        self.n = n_fields * ncp
        self.nnz = 0
        self.n_parts = 0
        self._h = C.c_uint64()
        check(lib.mfem_mesh_operator_create(ctx._h, dim, itp, nel, ncp, n_fields, _ptr(coords), _ptr(controlpoint_IDs), index_base, C.byref(self._h)))
        ctx._children.add(self)

    @staticmethod
    def _terms(terms):
        arr = (_lib.OperatorTerm * max(len(terms), 1))()
        for i, t in enumerate(terms):
            nrm = tuple(t[4]) if len(t) > 4 else (0.0, 0.0, 0.0)
            arr[i] = _lib.OperatorTerm(int(t[0]), int(t[1]), int(t[2]), 0, float(t[3]), (C.c_double * 3)(*[float(v) for v in nrm]))
        return arr

    def set_elements(self, itg: int, ref_itp_vals: torch.Tensor, itg_weight: torch.Tensor, adj_ptr: torch.Tensor, adj: torch.Tensor, terms) -> int:
        """rc of mfem_mesh_operator_set_elements (0, or -3 = MFEM_ERR_UNSUPPORTED: beyond the caps; anything else raises)."""
        rc = lib.mfem_mesh_operator_set_elements(self._h, itg, _ptr(ref_itp_vals), _ptr(itg_weight), _ptr(adj_ptr), _ptr(adj), len(terms),
                                                 self._terms(terms))
        if rc != -3:
            check(rc)
            self._keep += [ref_itp_vals, itg_weight, adj_ptr, adj]
            self.n_parts = max(self.n_parts, 1)
        return rc

    def add_facets(self, itg_b: int, n_face_ids: int, bdy_ref_itp_vals, bdy_itg_weights, bdy_tangent_directions, element_ID, element_eindex, adj_ptr,
                   adj, terms) -> int:
        """The part's number (>= 1), or -3 = MFEM_ERR_UNSUPPORTED."""
        part = C.c_int32(-1)
        rc = lib.mfem_mesh_operator_add_facets(self._h, itg_b, n_face_ids, element_ID.numel(), _ptr(bdy_ref_itp_vals), _ptr(bdy_itg_weights),
                                               _ptr(bdy_tangent_directions), _ptr(element_ID), _ptr(element_eindex), _ptr(adj_ptr), _ptr(adj),
                                               len(terms), self._terms(terms), C.byref(part))
        if rc == -3:
            return rc
        check(rc)
        self._keep += [bdy_ref_itp_vals, bdy_itg_weights, bdy_tangent_directions, element_ID, element_eindex, adj_ptr, adj]
        self.n_parts = part.value + 1
        return part.value

    def set_terms(self, part: int, terms) -> int:
        """Replaces the terms of a part (host only); rc as set_elements."""
        rc = lib.mfem_mesh_operator_set_terms(self._h, part, len(terms), self._terms(terms))
        if rc != -3:
            check(rc)
        return rc

    def set_variable_terms(self, part: int, terms, vals: Optional[torch.Tensor]) -> int:
        """Replaces the variable terms `(dual_sd, base_sd, block)` of a part (host only); vals: the float64 device array [n_terms, n_items, itg] of
        their coefficients (borrowed: read at every later product, diagonal and solve; rewrite its contents freely).  No terms: they are removed.
        rc as set_elements."""
        arr = (_lib.KvalTerm * max(len(terms), 1))(*[_lib.KvalTerm(int(t[0]), int(t[1]), int(t[2]), 0) for t in terms])
        rc = lib.mfem_mesh_operator_set_variable_terms(self._h, part, len(terms), arr, _ptr(vals) if len(terms) else None)
        if rc != -3:
            check(rc)
            self._var_keep[part] = vals if len(terms) else None
        return rc

    def mul_(self, y: torch.Tensor, x: torch.Tensor, alpha: float = 1.0, beta: float = 0.0) -> torch.Tensor:
        """y = alpha K x + beta y (beta == 0: y is not read)."""
        _need(x, torch.float64, "x", self.n)
        _need(y, torch.float64, "y", self.n)
        check(lib.mfem_mesh_operator_apply(self.ctx._h, self._h, _ptr(x), _ptr(y), alpha, beta))
        return y

    def diagonal(self) -> torch.Tensor:
        """diag K, signed (0 on a row without adjacency)."""
        d = torch.empty(self.n, dtype=torch.float64, device=f"cuda:{self.ctx.device}")
        check(lib.mfem_mesh_operator_diagonal(self.ctx._h, self._h, _ptr(d)))
        return d

    def close(self):
        if self._h:
            lib.mfem_mesh_operator_destroy(self._h)
            self._h = C.c_uint64()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BrickOperatorRefused(MetaFEMError):
    """mfem_brick_operator_create answered MFEM_ERR_UNSUPPORTED; the message is the library's."""


class BrickOperator:
    """Matrix-free K of a hex-8 thermal brick (mfem_brick_operator_*, csrc/brick_operator_thermal.hip): the matrix of Brick.assemble_thermal for the same
    parameters, evaluated from the brick's coordinates (read live: they may move between solves) -- no pattern, no values, no scratch.  Stands where
    a FEM_SpMat_CSR and its values stand: `mul_(b, op, None, x)` and `iterative_Solve(op, None, residue, ...)` take it.  Made by
    Brick.thermal_operator; raises BrickOperatorRefused (a MetaFEMError) with the library's message for a brick it refuses (hex-27, a slab)."""

    def __init__(self, brick: "Brick", params: "ThermalParams"):
        self.ctx, self.brick = brick.ctx, brick  # (the library borrows the brick: kept alive here)
        self.n = brick.ncp
        self.nnz = 0
        self._mg = None  # the BrickMultigrid made by multigrid(), if any (a solve's default hierarchy lives in the library alone)
        self._h = C.c_uint64()
        rc = lib.mfem_brick_operator_create(self.ctx._h, brick._h, C.byref(params), C.byref(self._h))
        if rc == -3:  # MFEM_ERR_UNSUPPORTED: a brick the operator does not cover
            raise BrickOperatorRefused(lib.mfem_last_error().decode())
        check(rc)
        self.params = params
        self.ctx._children.add(self)

    def set_params(self, k: float, h: float = 0.0, Tenv: float = 0.0, robin_faces: int = 0, fixed_faces: int = 0, h_penalty: float = 0.0,
                   Tw: float = 0.0):
        """Re-sends the parameters (host only, nothing is launched)."""
        p = ThermalParams(k, h, Tenv, robin_faces, fixed_faces, h_penalty, Tw)
        check(lib.mfem_brick_operator_set_params(self._h, C.byref(p)))
        self.params = p

    def mul_(self, y: torch.Tensor, x: torch.Tensor, alpha: float = 1.0, beta: float = 0.0) -> torch.Tensor:
        """y = alpha K x + beta y (beta == 0: y is not read)."""
        _need(x, torch.float64, "x", self.n)
        _need(y, torch.float64, "y", self.n)
        check(lib.mfem_brick_operator_apply(self.ctx._h, self._h, _ptr(x), _ptr(y), alpha, beta))
        return y

    def diagonal(self, preset: float = 1.0) -> torch.Tensor:
        """|diag K| under the guarded rule of jacobi_by_diagonal: a row with an exactly zero diagonal keeps `preset`."""
        d = torch.full((self.n,), float(preset), dtype=torch.float64, device=f"cuda:{self.ctx.device}")
        check(lib.mfem_brick_operator_diagonal(self.ctx._h, self._h, _ptr(d)))
        return d

    def multigrid(self, nonsymmetric: bool = False, **opts) -> "BrickMultigrid":
        """The geometric multigrid hierarchy of this operator (mfem_brick_multigrid_create): one per operator, destroyed with it.  opts:
        smoother_degree, coarse_degree, smoothing_range, coarse_range, eig_steps, max_levels (0 or absent: the default).  Raises MultigridRefused for
        an operator the hierarchy does not cover (an active Nitsche term; an ElasticityBrickOperator builds its own three-field hierarchy and
        refuses tau == 0 or no penalty face; a Hex27BrickOperator builds its own p-coarsened one and refuses a rule below itg_order 4).
        nonsymmetric = True (mfem_brick_multigrid_create_nonsymmetric, the hex-8 thermal operator only): the same hierarchy, created and set up
        with or without an active Nitsche (fixed_faces) term; with it attached iterative_Solve takes Sv_func = gmres_ with Pr_func = Pr_Multigrid_
        (cg_ as well while the Nitsche term is off)."""
        return BrickMultigrid(self, nonsymmetric=nonsymmetric, **opts)

    def close(self):
        if self._h:
            mg = getattr(self, "_mg", None)
            if mg is not None:  # (the library destroys the hierarchy with its operator)
                mg._h = C.c_uint64()
                self._mg = None
            lib.mfem_brick_operator_destroy(self._h)
            self._h = C.c_uint64()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultigridRefused(MetaFEMError):
    """mfem_brick_multigrid_create / _setup answered MFEM_ERR_UNSUPPORTED; the message is the library's."""


def multigrid_plan(n, max_levels: int = 12):
    """The level plan of an (nx, ny, nz) brick (csrc/brick_multigrid_decide.h: mg_plan): level l + 1 exists while all three element counts of level l
    are even and each half is >= 2."""
    levels = [tuple(int(v) for v in n)]
    while len(levels) < max_levels and all(v % 2 == 0 and v // 2 >= 2 for v in levels[-1]):
        levels.append(tuple(v // 2 for v in levels[-1]))
    return levels


def multigrid_plan_hex27(n, max_levels: int = 12):
    """The level plan of a hex-27 brick of (nx, ny, nz) elements (csrc/brick_multigrid_decide.h: mg_plan_hex27), in ELEMENT counts: level 0 is the
    hex-27 brick on the lattice 2 n + 1, level 1 -- whenever max_levels >= 2 -- a hex-8 brick of the same elements on the lattice n + 1
    (p-coarsening), then multigrid_plan's halving rule."""
    first = tuple(int(v) for v in n)
    return [first] + (multigrid_plan(first, max_levels - 1) if max_levels >= 2 else [])


class BrickMultigrid:
    """Geometric multigrid V-cycle of a hex-8 thermal BrickOperator, of an ElasticityBrickOperator or of a Hex27BrickOperator
    (mfem_brick_multigrid_*, csrc/brick_multigrid.hip): the preconditioner `iterative_Solve(op, None, b, tol, Sv_func=cg_, Pr_func=Pr_Multigrid_)`
    applies.  The operator says which entry point creates it (ElasticityBrickOperator: mfem_brick_multigrid_create_elasticity, three field-major
    fields per lattice point: apply() takes op.n = 3 * ncp entries; Hex27BrickOperator: mfem_brick_multigrid_create_hex27, level 1 is a hex-8
    brick of the same elements, so info()["ne"][0] == info()["ne"][1]).  A solve runs setup() itself, always; setup() and apply() are for a
    caller that uses the cycle on its own."""

    def __init__(self, op: "BrickOperator", nonsymmetric: bool = False, **opts):
        unknown = set(opts) - {"smoother_degree", "coarse_degree", "smoothing_range", "coarse_range", "eig_steps", "max_levels"}
        if unknown:
            raise TypeError(f"unknown multigrid options {sorted(unknown)}")
        self.ctx, self.op = op.ctx, op
        self._h = C.c_uint64()
        o = _lib.MultigridOptions(int(opts.get("smoother_degree", 0)), int(opts.get("coarse_degree", 0)), float(opts.get("smoothing_range", 0.0)),
                                  float(opts.get("coarse_range", 0.0)), int(opts.get("eig_steps", 0)), int(opts.get("max_levels", 0)))
        # (nonsymmetric: the library answers for an operator that entry point does not cover)
        create = getattr(lib, "mfem_brick_multigrid_create_nonsymmetric" if nonsymmetric else getattr(op, "_multigrid_create", "mfem_brick_multigrid_create"))
        rc = create(self.ctx._h, op._h, C.byref(o), C.byref(self._h))
        if rc == -3:
            raise MultigridRefused(lib.mfem_last_error().decode())
        check(rc)
        op._mg = self

    def setup(self):
        rc = lib.mfem_brick_multigrid_setup(self.ctx._h, self._h)
        if rc == -3:
            raise MultigridRefused(lib.mfem_last_error().decode())
        check(rc)
        return self

    def apply(self, r: torch.Tensor, z: Optional[torch.Tensor] = None) -> torch.Tensor:
        """z = one cycle applied to r (r is not changed)."""
        _need(r, torch.float64, "r", self.op.n)
        if z is None:
            z = torch.empty_like(r)
        _need(z, torch.float64, "z", self.op.n)
        check(lib.mfem_brick_multigrid_apply(self.ctx._h, self._h, _ptr(r), _ptr(z)))
        return z

    def info(self) -> dict:
        """levels, ne (element counts per level), lambda_max (per level, without the 1.1), sign, bytes, cycles, setups, products (per level, the
        cycles' only), setup_products."""
        i = _lib.MultigridInfo()
        check(lib.mfem_brick_multigrid_info(self._h, C.byref(i)))
        L = i.levels
        return dict(levels=L, sign=i.sign, ne=[(i.nx[l], i.ny[l], i.nz[l]) for l in range(L)], lambda_max=[i.lambda_max[l] for l in range(L)],
                    products=[i.products[l] for l in range(L)], setup_products=i.setup_products, bytes=i.bytes, cycles=i.cycles, setups=i.setups,
                    nonsymmetric=lib.mfem_brick_multigrid_nonsymmetric(self._h) == 1)

    def close(self):
        if self._h:
            lib.mfem_brick_multigrid_destroy(self._h)
            self._h = C.c_uint64()
            if getattr(self.op, "_mg", None) is self:
                self.op._mg = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ElasticityBrickOperator(BrickOperator):
    """Matrix-free K of a hex-8 brick under three-field linear elasticity (mfem_brick_operator_create_elasticity, csrc/brick_operator_elasticity.hip):
    the matrix of Brick.assemble_elasticity for the same parameters -- the volume term and the penalty faces; traction faces and sig are the
    residual's load and do not enter K.  n = 3 * ncp, field-major.  Made by Brick.elasticity_operator; mul_, diagonal and iterative_Solve take it
    as they take a BrickOperator.  multigrid(**opts) attaches a three-field hierarchy (mfem_brick_multigrid_create_elasticity): with one attached,
    and only then, iterative_Solve takes Pr_func = Pr_Multigrid_ with cg_; it raises MultigridRefused for tau == 0 or no penalty face (K is
    singular)."""

    _multigrid_create = "mfem_brick_multigrid_create_elasticity"  # (BrickMultigrid asks the operator which entry point builds its hierarchy)

    def __init__(self, brick: "Brick", params: "ElasticityParams"):
        self.ctx, self.brick = brick.ctx, brick  # (the library borrows the brick: kept alive here)
        self.n = 3 * brick.ncp
        self.nnz = 0
        self._mg = None
        self._h = C.c_uint64()
        rc = lib.mfem_brick_operator_create_elasticity(self.ctx._h, brick._h, C.byref(params), C.byref(self._h))
        if rc == -3:  # MFEM_ERR_UNSUPPORTED: a brick the operator does not cover
            raise BrickOperatorRefused(lib.mfem_last_error().decode())
        check(rc)
        self.params = params
        self.ctx._children.add(self)

    def set_params(self, lam: float, mu: float, tau: float = 0.0, penalty_faces: int = 0):
        """Re-sends the parameters (host only, nothing is launched)."""
        p = ElasticityParams(lam, mu, tau, penalty_faces, 0, (C.c_double * 6)(*([0.0] * 6)))
        check(lib.mfem_brick_operator_set_elasticity_params(self._h, C.byref(p)))
        self.params = p


class Hex27BrickOperator(BrickOperator):
    """Matrix-free K of a hex-27 (order-2) thermal brick (mfem_brick_operator_create_hex27, csrc/brick_operator_hex27.hip): the matrix of
    Brick.assemble_thermal for the same parameters -- volume term, Robin faces, Nitsche fixed_faces -- evaluated from the coordinates by a row-owner
    sweep; n = ncp.  Made by Brick.thermal_operator_hex27; set_params, mul_, diagonal and iterative_Solve take it as they take a BrickOperator.
    Raises BrickOperatorRefused for a hex-8 brick (Brick.thermal_operator covers it) and for a brick with a slab.  multigrid(**opts) attaches a
    hierarchy (mfem_brick_multigrid_create_hex27: p-coarsening onto a hex-8 brick of the same elements, then the hex-8 thermal hierarchy): with one
    attached, and only then, iterative_Solve takes Pr_func = Pr_Multigrid_ with cg_; it raises MultigridRefused for an active Nitsche term and for a
    rule with fewer than 3 Gauss points per direction (itg_order < 4: the under-integrated K keeps near-null modes the coarse space does not hold)."""

    def __init__(self, brick: "Brick", params: "ThermalParams"):
        self.ctx, self.brick = brick.ctx, brick  # (the library borrows the brick: kept alive here)
        self.n = brick.ncp
        self.nnz = 0
        self._mg = None
        # (BrickMultigrid asks the operator which entry point builds its hierarchy.  Set on the operator, not on the class: the class keeps answering
        # hasattr(Hex27BrickOperator, "_multigrid_create") with False, which tests/test_brick_multigrid_elasticity_host.py pins)
        self._multigrid_create = "mfem_brick_multigrid_create_hex27"
        self._h = C.c_uint64()
        rc = lib.mfem_brick_operator_create_hex27(self.ctx._h, brick._h, C.byref(params), C.byref(self._h))
        if rc == -3:  # MFEM_ERR_UNSUPPORTED: a brick the operator does not cover
            raise BrickOperatorRefused(lib.mfem_last_error().decode())
        check(rc)
        self.params = params
        self.ctx._children.add(self)


class Hex27ElasticityBrickOperator(BrickOperator):
    """Matrix-free K of a hex-27 (order-2) brick under three-field linear elasticity (mfem_brick_operator_create_elasticity_hex27,
    csrc/brick_operator_elasticity_hex27.hip): the cantilever form's volume term and penalty faces, evaluated from the coordinates by the row-owner
    sweep of the hex-27 thermal operator with three fields; n = 3 * ncp, field-major.  traction_faces and sig do not enter K: they are the load of
    residual().  Made by Brick.elasticity_operator_hex27; mul_, diagonal and iterative_Solve take it as they take a BrickOperator.  Raises
    BrickOperatorRefused for a hex-8 brick (Brick.elasticity_operator covers it), a brick with a slab and a rule whose LDS block does not fit
    (brick_operator_elasticity_hex27_refusal).  multigrid() raises MultigridRefused: a hierarchy for it does not exist yet."""

    def __init__(self, brick: "Brick", params: "ElasticityParams"):
        self.ctx, self.brick = brick.ctx, brick  # (the library borrows the brick: kept alive here)
        self.n = 3 * brick.ncp
        self.nnz = 0
        self._mg = None
        self._h = C.c_uint64()
        rc = lib.mfem_brick_operator_create_elasticity_hex27(self.ctx._h, brick._h, C.byref(params), C.byref(self._h))
        if rc == -3:  # MFEM_ERR_UNSUPPORTED: a brick the operator does not cover
            raise BrickOperatorRefused(lib.mfem_last_error().decode())
        check(rc)
        self.params = params
        self.ctx._children.add(self)

    def set_params(self, lam: float, mu: float, tau: float = 0.0, penalty_faces: int = 0, traction_faces: int = 0, sig=(0.0,) * 6):
        """Re-sends the parameters, the residual's load included (host only, nothing is launched)."""
        p = ElasticityParams(lam, mu, tau, penalty_faces, traction_faces, (C.c_double * 6)(*sig))
        check(lib.mfem_brick_operator_set_elasticity_params(self._h, C.byref(p)))
        self.params = p

    def residual(self, x_star: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """K_nonlinear_func of the form: K x_star + f, f the traction sig on traction_faces (mfem_brick_operator_residual_elasticity)."""
        _need(x_star, torch.float64, "x_star", self.n)
        res = out if out is not None else torch.empty(self.n, dtype=torch.float64, device=x_star.device)
        _need(res, torch.float64, "out", self.n)
        check(lib.mfem_brick_operator_residual_elasticity(self.ctx._h, self._h, _ptr(x_star), _ptr(res)))
        return res


_OPERATORS = (MeshOperator, BrickOperator, Hex27BrickOperator, Hex27ElasticityBrickOperator)  # what stands in for (A, vals) with vals = None


def mul_(b: torch.Tensor, A, vals: Optional[torch.Tensor], x: torch.Tensor, alpha: float = 1.0, beta: float = 0.0):
    """mul!(b, A, x, alpha, beta): b = alpha*A*x + beta*b (04_GPU_Utils.jl:131).  A MeshOperator or BrickOperator takes vals = None."""
    if isinstance(A, _OPERATORS):
        if vals is not None:
            raise MetaFEMError(f"a {type(A).__name__} holds no values: pass vals = None")
        return A.mul_(b, x, alpha, beta)
    _need(vals, torch.float64, "vals", A.nnz)
    _need(x, torch.float64, "x")
    _need(b, torch.float64, "b", A.n)
    check(lib.mfem_spmv_csr(A.ctx._h, A._h, _ptr(vals), _ptr(x), _ptr(b), alpha, beta))
    return b


def tmul_(b: torch.Tensor, A: FEM_SpMat_CSR, vals: torch.Tensor, x: torch.Tensor, alpha: float = 1.0, beta: float = 0.0):
    """tmul!(b, A, x): b = alpha*A'*x + beta*b (04_GPU_Utils.jl:132, CUSPARSE mv! 'T').  x has A.n entries, b has A.ncols.
    The first call transposes the pattern on the device and caches the plan on the handle (replan() drops it)."""
    _need(vals, torch.float64, "vals", A.nnz)
    _need(x, torch.float64, "x", A.n)
    _need(b, torch.float64, "b", A.ncols)
    check(lib.mfem_spmv_csr_t(A.ctx._h, A._h, _ptr(vals), _ptr(x), _ptr(b), alpha, beta))
    return b


def dot(x: torch.Tensor, y: torch.Tensor, ctx: Optional[Context] = None) -> float:
    ctx = ctx or default_context()
    _need(x, torch.float64, "x")
    _need(y, torch.float64, "y", x.numel())
    out = C.c_double()
    check(lib.mfem_dot(ctx._h, x.numel(), _ptr(x), _ptr(y), C.byref(out)))
    return out.value


def nrm2(x: torch.Tensor, ctx: Optional[Context] = None) -> float:
    ctx = ctx or default_context()
    _need(x, torch.float64, "x")
    out = C.c_double()
    check(lib.mfem_nrm2(ctx._h, x.numel(), _ptr(x), C.byref(out)))
    return out.value


def normalized_norm(x: torch.Tensor, ctx: Optional[Context] = None) -> float:
    """normalized_norm(x) = norm(x)/sqrt(length(x)) (04_Time_Domain.jl:51)."""
    return nrm2(x, ctx) / math.sqrt(x.numel())


def axpby_(a: float, x: torch.Tensor, b: float, y: torch.Tensor, ctx: Optional[Context] = None):
    ctx = ctx or default_context()
    _need(x, torch.float64, "x")
    _need(y, torch.float64, "y", x.numel())
    check(lib.mfem_axpby(ctx._h, x.numel(), a, _ptr(x), b, _ptr(y)))
    return y


def FEM_rand(n: int, seed: int = 0x5EED, stream_id: int = 0, ctx: Optional[Context] = None) -> torch.Tensor:
    """FEM_rand (04_GPU_Utils.jl:22) with an explicit seed (the reference's stream is unseeded, F9)."""
    ctx = ctx or default_context()
    x = torch.empty(n, dtype=torch.float64, device=f"cuda:{ctx.device}")
    check(lib.mfem_rand(ctx._h, n, seed, stream_id, _ptr(x)))
    return x


def jacobi_by_diagonal(A: FEM_SpMat_CSR, vals: torch.Tensor) -> torch.Tensor:
    """d has A.ncols entries (owned | ghost columns of a slab pattern, the ghost part left at 1: fill it with halo_)."""
    d = torch.ones(A.ncols, dtype=torch.float64, device=vals.device)
    check(lib.mfem_jacobi_by_diagonal(A.ctx._h, A._h, _ptr(vals), _ptr(d)))
    return d


def jacobi2_by_column(A: FEM_SpMat_CSR, vals: torch.Tensor) -> torch.Tensor:
    """Column 2-norms, A.ncols entries.  On a slab pattern with a communicator attached the ghost-column contributions go to
    their owners (mfem_halo_reduce) and the ghost entries come back as the owners' values: the GLOBAL column norms."""
    d = torch.zeros(A.ncols, dtype=torch.float64, device=vals.device)
    check(lib.mfem_jacobi2_by_column(A.ctx._h, A._h, _ptr(vals), _ptr(d)))
    return d


def jacobi_by_row(A: FEM_SpMat_CSR, vals: torch.Tensor) -> torch.Tensor:
    d = torch.zeros(A.n, dtype=torch.float64, device=vals.device)
    check(lib.mfem_jacobi_by_row(A.ctx._h, A._h, _ptr(vals), _ptr(d)))
    return d


def mat_div_jacobi_(A: FEM_SpMat_CSR, vals: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    check(lib.mfem_mat_div_jacobi(A.ctx._h, A._h, _ptr(vals), _ptr(d)))
    return vals


def iterative_Solve(A, K_vals: Optional[torch.Tensor], residue: torch.Tensor, converge_tol: float, *,
                    Sv_func: int = idrs_, Pr_func: int = Pr_Jacobi_, Pl_func: int = Identity, max_pass: int = 4,
                    maxiter: int = 2000,
                    s: int = 0, seed: int = 0x5EED, check_every: int = 32, fixed_iterations: bool = False,
                    scale_in_place: bool = False, shadow: Optional[torch.Tensor] = None, cg_variant: int = 0,
                    checkiter: int = 200) -> Tuple[torch.Tensor, SolveStats]:
    """iterative_Solve!(globalfield; Sv_func!, Pr_func!, Pl_func, max_pass, maxiter, s) (02_Preconditioner.jl:32-76).
    Sv_func: cg_ (added), bicgstabl_GS_ (03_BiCGstabl.jl), idrs_ (04_IDRs.jl), cgs2_ (07_CGS.jl:54-105), gmres_ (05_GMRES.jl:48-100: restarted
    GMRES), cgs_ (07_CGS.jl:13-52), tfqmr_ (08_QMR.jl:3-74) or lsqr_ (06_LSQR.jl:10-70: products with A and A'); the last four on one
    rank only.  s: BiCGStab l (0: 2), IDR s (0: 4) or the GMRES restart length (0: 20, the reference's default); at most 32.
    checkiter (tfqmr_ only, the reference's kwarg, default 200): the true residual is tested every checkiter iterations.
    Pl_func: Identity, Pl_Jacobi_ (:155-168) or Pl_Jacobi_rownorm_ (normalized_by_row = true).
    cg_variant (cg_ only): 0 auto, 1 classic recurrence, 2 single reduction group per iteration (Chronopoulos-Gear), 3 classic
    recurrence carrying the preconditioned residual (one vector stream less per iteration), 4 plain CG on the symmetrically Jacobi-scaled
    matrix (one stream less again; on the mirrored-sweep layout, one rank: the auto choice there, else 3).

    A MeshOperator or a BrickOperator with K_vals = None solves matrix-free (mfem_solve_operator): every Sv_func but lsqr_, Pr_func Identity or Pr_Jacobi_, Pl_func
    Identity, no scale_in_place.  Pr_func = Pr_Multigrid_: a geometric multigrid V-cycle, for Sv_func = cg_ on a hex-8 thermal BrickOperator
    without an active Nitsche term and without a communicator (anything else raises with the library's reason); the solve creates a default hierarchy
    when BrickOperator.multigrid has not made one and always runs its setup first (inside solve_ms); check_every and cg_variant are ignored.
    An ElasticityBrickOperator takes it under the same conditions once ElasticityBrickOperator.multigrid() has attached a hierarchy (that call is
    the opt-in: without it the solve raises and the message names the entry point) and while tau != 0 on at least one penalty face; a
    Hex27BrickOperator likewise once Hex27BrickOperator.multigrid() has attached one (refused with an active Nitsche term or itg_order < 4).
    Sv_func = gmres_ takes Pr_Multigrid_ on a hex-8 thermal BrickOperator once BrickOperator.multigrid(nonsymmetric=True) has attached a hierarchy,
    with or without an active Nitsche term: right-preconditioned restarted GMRES(s), one V-cycle per Arnoldi step and one per restart; stats.iterations
    counts Arnoldi steps.

    Returns (delta_x, stats); delta_x is a NEW device vector like the reference's return value.
    """
    matrix_free = isinstance(A, _OPERATORS)
    if matrix_free and K_vals is not None:
        raise MetaFEMError(f"a {type(A).__name__} holds no values: pass K_vals = None")
    if not matrix_free:
        _need(K_vals, torch.float64, "K_vals", A.nnz)
    _need(residue, torch.float64, "residue", A.n)
    x = torch.empty(A.n, dtype=torch.float64, device=residue.device)
    if Sv_func == tfqmr_:
        if checkiter < 1:
            raise MetaFEMError("checkiter must be >= 1")
        s = checkiter
    o = SolveOptions(method=Sv_func, precond=Pr_func, l_or_s=s, maxiter=maxiter, max_pass=max_pass,
                     check_every=check_every, converge_tol=converge_tol, seed=seed,
                     fixed_iterations=1 if fixed_iterations else 0, scale_in_place=1 if scale_in_place else 0,
                     left_precond=Pl_func, cg_variant=cg_variant)
    st = SolveStats()
    if shadow is not None:
        _need(shadow, torch.float64, "shadow")
        check(lib.mfem_solve_set_shadow(A.ctx._h, _ptr(shadow), shadow.numel() // A.n))
    try:
        if matrix_free:
            check(lib.mfem_solve_operator(A.ctx._h, A._h, _ptr(residue), _ptr(x), C.byref(o), C.byref(st)))
        else:
            check(lib.mfem_solve(A.ctx._h, A._h, _ptr(K_vals), _ptr(residue), _ptr(x), C.byref(o), C.byref(st)))
    finally:
        if shadow is not None:
            lib.mfem_solve_set_shadow(A.ctx._h, None, 0)
    return x, st


def assemble_SparseID(controlpoint_IDs: torch.Tensor, ncp: int, n_fields: int = 1, index_base: int = 1,
                      with_slots: bool = True, ctx: Optional[Context] = None):
    """assemble_SparseID! (03_GlobalAssembly.jl:77-140) for unstructured connectivity.
    controlpoint_IDs: int32 device tensor of shape (nel, itp) in C order == [itp, nel] column-major.
    Returns (FEM_SpMat_CSR, sparse_IDs_by_el) with sparse_IDs_by_el of shape (n_fields^2, nel, itp_b, itp_a)."""
    ctx = ctx or default_context()
    _need(controlpoint_IDs, torch.int32, "controlpoint_IDs")
    nel, itp = controlpoint_IDs.shape
    slots = torch.empty((n_fields * n_fields, nel, itp, itp), dtype=torch.int32, device=controlpoint_IDs.device) if with_slots else None
    h = C.c_void_p()
    check(lib.mfem_pattern_build(ctx._h, itp, nel, ncp, _ptr(controlpoint_IDs), index_base, n_fields, C.byref(h), _ptr(slots)))
    A = FEM_SpMat_CSR.__new__(FEM_SpMat_CSR)
    A.ctx, A._h, A._owned, A.index_base = ctx, h, True, 0
    A.n, A.nnz = int(lib.mfem_csr_n(h)), int(lib.mfem_csr_nnz(h))
    A.rowptr = _tensor_from_ptr(lib.mfem_csr_rowptr64(h), A.n + 1, torch.int64, ctx.device, owner=A)
    A.colidx = _tensor_from_ptr(lib.mfem_csr_colidx(h), A.nnz, torch.int32, ctx.device, owner=A)
    ctx._children.add(A)
    return A, slots


def _op_layout(itg, itp, n_sd, n_host, index_base, colour_offsets):
    if colour_offsets is None:
        return OpLayout(itg, itp, n_sd, n_host, index_base, 0, None), None
    arr = (C.c_int64 * len(colour_offsets))(*[int(v) for v in colour_offsets])
    return OpLayout(itg, itp, n_sd, n_host, index_base, len(colour_offsets) - 1, arr), arr


def _Var_Basic(itp_vals, sd, cpID_shift, el_g_cpIDs, x, target, itg_hostIDs, elIDs, *, dims, index_base=1, ctx=None):
    """_Var_Basic(itp_vals, sd_IDs, cpID_shift, el_g_cpIDs, x_star, target, itg_hostIDs, elIDs) (06_FEM_Kernel.jl:1-13).
    dims = (itg, itp, n_sd, n_host); `sd` is the flat 0-based slot of the reference's sd_IDs tuple."""
    ctx = ctx or default_context()
    L, _keep = _op_layout(*dims, index_base, None)
    check(lib.mfem_op_var(ctx._h, C.byref(L), _ptr(itp_vals), sd, cpID_shift, _ptr(el_g_cpIDs), _ptr(x), _ptr(target),
                          _ptr(itg_hostIDs), _ptr(elIDs), elIDs.numel()))
    return target


def _Kval_Basic(itp_vals, dual_sd, base_sd, vals, sparse_IDs_by_el, sparse_ID_shift, K_val, itg_hostIDs, elIDs, *, dims,
                index_base=1, colour_offsets=None, ctx=None):
    """_Kval_Basic(...) (06_FEM_Kernel.jl:28-45); colour_offsets = None -> FP64 atomics like the reference."""
    ctx = ctx or default_context()
    L, _keep = _op_layout(*dims, index_base, colour_offsets)
    check(lib.mfem_op_kval(ctx._h, C.byref(L), _ptr(itp_vals), dual_sd, base_sd, _ptr(vals), _ptr(sparse_IDs_by_el),
                           sparse_ID_shift, _ptr(K_val), _ptr(itg_hostIDs), _ptr(elIDs), elIDs.numel()))
    return K_val


def _Res_Basic(itp_vals, dual_sd, vals, cpID_shift, el_g_cpIDs, residue, itg_hostIDs, elIDs, *, dims, index_base=1,
               colour_offsets=None, ctx=None):
    """_Res_Basic(...) (06_FEM_Kernel.jl:65-79)."""
    ctx = ctx or default_context()
    L, _keep = _op_layout(*dims, index_base, colour_offsets)
    check(lib.mfem_op_res(ctx._h, C.byref(L), _ptr(itp_vals), dual_sd, _ptr(vals), cpID_shift, _ptr(el_g_cpIDs),
                          _ptr(residue), _ptr(itg_hostIDs), _ptr(elIDs), elIDs.numel()))
    return residue


class Brick:
    """make_Brick(x, n, :CUBE) + mesh_Classical(itp_type=:Lagrange, itp_order, itg_order) + update_Mesh
    on device (201_Helper_TM.jl:36-51; 2_Interface.jl:7,98-108)."""

    def __init__(self, x: Tuple[float, float, float], n: Tuple[int, int, int], itp_order: int = 1, itg_order: int = 3,
                 ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()
        self.x, self.n, self.itp_order, self.itg_order = tuple(x), tuple(n), itp_order, itg_order
        self._h = C.c_void_p()
        check(lib.mfem_brick_create(self.ctx._h, n[0], n[1], n[2], x[0], x[1], x[2], itp_order, itg_order, C.byref(self._h)))
        self.ncp = int(lib.mfem_brick_num_controlpoints(self._h))
        self.nel = int(lib.mfem_brick_num_elements(self._h))
        self.m = tuple(itp_order * ni + 1 for ni in n)
        self.slab = (0, self.m[0])
        self.ctx._children.add(self)

    def set_slab(self, plane_lo: int, plane_hi: int):
        check(lib.mfem_brick_set_slab(self._h, plane_lo, plane_hi))
        self.slab = (plane_lo, plane_hi)

    @property
    def n_owned(self) -> int:
        return (self.slab[1] - self.slab[0]) * self.m[1] * self.m[2]

    def coords_view(self, d: int) -> torch.Tensor:
        """Device view of controlpoints.x{d+1} (library-owned memory) as a torch tensor."""
        gw = self.itp_order  # ghost planes per side
        clo = max(self.slab[0] - gw, 0) if self.slab != (0, self.m[0]) else 0
        chi = min(self.slab[1] + gw, self.m[0]) if self.slab != (0, self.m[0]) else self.m[0]
        ncoord = (chi - clo) * self.m[1] * self.m[2]
        ptr = lib.mfem_brick_coords(self._h, d)
        return _tensor_from_ptr(ptr, ncoord, torch.float64, self.ctx.device, owner=self)

    def pattern(self, n_fields: int = 1) -> FEM_SpMat_CSR:
        """assemble_SparseID! (03_GlobalAssembly.jl:77-140) -> row-sorted CSR, K_val_ids = identity."""
        h = C.c_void_p()
        check(lib.mfem_brick_pattern(self.ctx._h, self._h, n_fields, C.byref(h)))
        n = int(lib.mfem_csr_n(h))
        nnz = int(lib.mfem_csr_nnz(h))
        A = FEM_SpMat_CSR.__new__(FEM_SpMat_CSR)
        A.ctx, A._h, A._owned, A.n, A.nnz, A.index_base = self.ctx, h, True, n, nnz, 0
        A.rowptr = _tensor_from_ptr(lib.mfem_csr_rowptr64(h), n + 1, torch.int64, self.ctx.device, owner=A)
        A.colidx = _tensor_from_ptr(lib.mfem_csr_colidx(h), nnz, torch.int32, self.ctx.device, owner=A)
        self.ctx._children.add(A)
        return A

    def assemble_thermal(self, A: FEM_SpMat_CSR, k: float, h: float = 0.0, Tenv: float = 0.0,
                         robin_faces: int = 0, out: Optional[torch.Tensor] = None, *, fixed_faces: int = 0,
                         h_penalty: float = 0.0, Tw: float = 0.0) -> torch.Tensor:
        """K_linear_func of -k*Bilinear(T{;i},T{;i}) + h*Bilinear(T, Tenv - T) on robin_faces
        (examples/thermal_conduction/3D_Script.jl:30-31) + the weakly imposed Dirichlet faces
        h_penalty*Bilinear(T, Tw - T) + k*Bilinear(T, n{i}*T{;i}) on fixed_faces (2D_Script.jl:58; K is nonsymmetric then)."""
        vals = out if out is not None else torch.empty(A.nnz, dtype=torch.float64, device=f"cuda:{self.ctx.device}")
        p = ThermalParams(k, h, Tenv, robin_faces, fixed_faces, h_penalty, Tw)
        check(lib.mfem_brick_assemble_thermal(self.ctx._h, self._h, A._h, C.byref(p), _ptr(vals)))
        return vals

    def thermal_operator(self, k: float, h: float = 0.0, Tenv: float = 0.0, robin_faces: int = 0, fixed_faces: int = 0, h_penalty: float = 0.0,
                         Tw: float = 0.0) -> "BrickOperator":
        """The matrix-free K of assemble_thermal for the same parameters (BrickOperator).  A hex-27 brick or a brick with a slab raises
        BrickOperatorRefused."""
        return BrickOperator(self, ThermalParams(k, h, Tenv, robin_faces, fixed_faces, h_penalty, Tw))

    def thermal_operator_hex27(self, k: float, h: float = 0.0, Tenv: float = 0.0, robin_faces: int = 0, fixed_faces: int = 0, h_penalty: float = 0.0,
                               Tw: float = 0.0) -> "Hex27BrickOperator":
        """The matrix-free K of assemble_thermal on an order-2 (hex-27) brick (Hex27BrickOperator).  A hex-8 brick or a brick with a slab raises
        BrickOperatorRefused."""
        return Hex27BrickOperator(self, ThermalParams(k, h, Tenv, robin_faces, fixed_faces, h_penalty, Tw))

    def residual_thermal(self, x_star: torch.Tensor, k: float, h: float = 0.0, Tenv: float = 0.0, robin_faces: int = 0,
                         s: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, *, fixed_faces: int = 0,
                         h_penalty: float = 0.0, Tw: float = 0.0) -> torch.Tensor:
        _need(x_star, torch.float64, "x_star", self.n_owned)
        res = out if out is not None else torch.empty(self.n_owned, dtype=torch.float64, device=x_star.device)
        p = ThermalParams(k, h, Tenv, robin_faces, fixed_faces, h_penalty, Tw)
        check(lib.mfem_brick_residual_thermal(self.ctx._h, self._h, C.byref(p), _ptr(x_star), _ptr(s), _ptr(res)))
        return res

    def assemble_elasticity(self, A: FEM_SpMat_CSR, lam: float, mu: float, tau: float = 0.0, penalty_faces: int = 0,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """K_linear_func of -Bilinear(eps{i,j}, sigma{i,j}) + tau*Bilinear(d{i}, dw{i} - d{i}), dw = 0
        (examples/linear_elasticity/cantilever/3D_Script.jl:52-60): the reference's 21 + 3 _Kval_Basic launches."""
        vals = out if out is not None else torch.empty(A.nnz, dtype=torch.float64, device=f"cuda:{self.ctx.device}")
        p = ElasticityParams(lam, mu, tau, penalty_faces, 0, (C.c_double * 6)(*([0.0] * 6)))
        check(lib.mfem_brick_assemble_elasticity(self.ctx._h, self._h, A._h, C.byref(p), _ptr(vals)))
        return vals

    def elasticity_operator(self, lam: float, mu: float, tau: float = 0.0, penalty_faces: int = 0) -> "ElasticityBrickOperator":
        """The matrix-free K of assemble_elasticity for the same parameters (a BrickOperator with n == 3 * ncp).  A hex-27 brick or a brick with a
        slab raises BrickOperatorRefused."""
        return ElasticityBrickOperator(self, ElasticityParams(lam, mu, tau, penalty_faces, 0, (C.c_double * 6)(*([0.0] * 6))))

    def elasticity_operator_hex27(self, lam: float, mu: float, tau: float = 0.0, penalty_faces: int = 0, traction_faces: int = 0,
                                  sig=(0.0,) * 6) -> "Hex27ElasticityBrickOperator":
        """The matrix-free K of the cantilever form on an order-2 brick (a BrickOperator with n == 3 * ncp); traction_faces and sig are kept for
        its residual().  A hex-8 brick, a brick with a slab or a rule the kernel does not serve raises BrickOperatorRefused."""
        return Hex27ElasticityBrickOperator(self, ElasticityParams(lam, mu, tau, penalty_faces, traction_faces, (C.c_double * 6)(*sig)))

    def residual_elasticity(self, x_star: torch.Tensor, lam: float, mu: float, tau: float = 0.0, penalty_faces: int = 0,
                            traction_faces: int = 0, sig=(0.0,) * 6, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """sig = constant symmetric tensor (11, 22, 33, 23, 13, 12) of Bilinear(d{i}, sig{i,j}*n{j}) (:61)."""
        _need(x_star, torch.float64, "x_star", 3 * self.n_owned)
        res = out if out is not None else torch.empty(3 * self.n_owned, dtype=torch.float64, device=x_star.device)
        p = ElasticityParams(lam, mu, tau, penalty_faces, traction_faces, (C.c_double * 6)(*sig))
        check(lib.mfem_brick_residual_elasticity(self.ctx._h, self._h, C.byref(p), _ptr(x_star), _ptr(res)))
        return res

    def close(self):
        if self._h:
            lib.mfem_brick_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def brick_operator_refusal(brick: Brick) -> Optional[str]:
    """The host's forecast of mfem_brick_operator_create's refusals (csrc/brick_operator_decide.h: bop_refusal), or None: lets ThermalDomain decide
    without a device call.  The library has the last word: ThermalDomain also falls back on BrickOperatorRefused."""
    if brick.itp_order != 1:
        return "an order-2 (hex-27) brick: the matrix-free brick operator covers hex-8 bricks"
    if tuple(brick.slab) != (0, brick.m[0]):
        return "a brick with a slab set: the matrix-free brick operator runs on the whole lattice, one rank"
    return None


def brick_operator_hex27_refusal(brick: Brick) -> Optional[str]:
    """The host's forecast of mfem_brick_operator_create_hex27's refusals (csrc/brick_operator_hex27_decide.h: bop27_refusal), or None."""
    if brick.itp_order != 2:
        return "an order-1 (hex-8) brick: the hex-27 operator covers order-2 bricks; a hex-8 brick takes mfem_brick_operator_create"
    if tuple(brick.slab) != (0, brick.m[0]):
        return "a brick with a slab set: the matrix-free brick operator runs on the whole lattice, one rank"
    return None


def _e27_constants():
    """the constants and the LDS arithmetic of csrc/brick_operator_elasticity_hex27_decide.h, restated (tests compare them with the header)"""
    return dict(NI=6, NF=3, TE=8, WAVES_MAX=12, WAVES_MIN=5, LDS_LIMIT=160 * 1024, LDS_STATIC=128)


def brick_operator_elasticity_hex27_lds_bytes(ng: int, waves: int) -> int:
    """e27_lds_bytes(ng, waves) of csrc/brick_operator_elasticity_hex27_decide.h: the volume kernel's dynamic LDS block of a workgroup of `waves`
    waves (a CU must hold it plus the kernel's 128 static bytes)."""
    c = _e27_constants()
    pad = lambda v: (v + 1) & ~1
    ni, nf, eh = c["NI"], c["NF"], c["TE"] + 1
    nq = ng ** 3
    n1, n2, n3, na, nb = 18 * ng * ni, 9 * ng * ng * ni, 18 * nq, nf * 9 * ng * ng, nf * 18 * ng
    w_t2 = pad(max(27 * ni + n1, n3, pad(na) + nb))
    w_size = w_t2 + pad(max(n2, 9 * nq)) + pad(nq)
    off_waves = pad(nq) + 8 * ng + (pad(n1 + n2 + n3 + na + nb) >> 1) + pad(eh * eh * 27 * nf)
    return 8 * (off_waves + waves * w_size)


def brick_operator_elasticity_hex27_waves(ng: int) -> int:
    """e27_waves(ng): waves per workgroup of a rule (as many as fit the LDS, 12 at the most), 0 when not even 5 fit."""
    c = _e27_constants()
    w = c["WAVES_MAX"]
    while w >= c["WAVES_MIN"] and brick_operator_elasticity_hex27_lds_bytes(ng, w) + c["LDS_STATIC"] > c["LDS_LIMIT"]:
        w -= 1
    return w if w >= c["WAVES_MIN"] else 0


def brick_operator_elasticity_hex27_refusal(brick: Brick) -> Optional[str]:
    """The host's forecast of mfem_brick_operator_create_elasticity_hex27's refusals (csrc/brick_operator_elasticity_hex27_decide.h:
    bop_e27_refusal, the rule predicate e27_rule_served included), or None."""
    if brick.itp_order != 2:
        return "an order-1 (hex-8) brick: the hex-27 elasticity operator covers order-2 bricks; a hex-8 brick takes mfem_brick_operator_create_elasticity"
    if tuple(brick.slab) != (0, brick.m[0]):
        return "a brick with a slab set: the matrix-free brick operator runs on the whole lattice, one rank"
    ng = brick.itg_order // 2 + 1
    if not 1 <= ng <= 4:
        return "a Gauss rule outside 1 to 4 points per direction (itg_order 1 to 7): the hex-27 tables hold no such rule"
    if brick_operator_elasticity_hex27_waves(ng) == 0:
        return "the 4-point Gauss rule (itg_order 6 to 7): the volume kernel's per-workgroup LDS block exceeds the 160 KB of a CU"
    return None


def make_Brick(x, n, itp_order: int = 1, itg_order: int = 3, ctx: Optional[Context] = None) -> Brick:
    return Brick(x, n, itp_order, itg_order, ctx)


class _PtrHolder:
    """__cuda_array_interface__ shim so torch can wrap library-owned device memory without copying."""

    def __init__(self, ptr: int, n: int, typestr: str, owner):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}
        self._owner = owner


def _tensor_from_ptr(ptr, n: int, dtype, device: int, owner=None) -> torch.Tensor:
    if n == 0 or not ptr:
        return torch.empty(0, dtype=dtype, device=f"cuda:{device}")
    typestr = {torch.float64: "<f8", torch.int64: "<i8", torch.int32: "<i4"}[dtype]
    return torch.as_tensor(_PtrHolder(int(ptr), n, typestr, owner), device=f"cuda:{device}")


class ElasticityDomain:
    """FEM_Domain + GlobalField for the linear-elasticity weak form of examples/linear_elasticity/cantilever/3D_Script.jl:52-61 on a structured
    brick (three fields, field-major): displacement held by the penalty tau on penalty_faces, the constant traction sig on traction_faces.  The two
    generated closures are the fused HIP kernels; update_OneStep is the reference's Newton driver, as in ThermalDomain."""

    def __init__(self, brick: Brick, lam: float, mu: float, tau: float, penalty_faces: int, traction_faces: int = 0, sig=(0.0,) * 6, *,
                 matrix_free=False, multigrid: bool = False):
        self.brick, self.lam, self.mu, self.tau, self.penalty_faces = brick, lam, mu, tau, penalty_faces
        self.traction_faces, self.sig = traction_faces, tuple(sig)
        dev = f"cuda:{brick.ctx.device}"
        # matrix_free = "any" (ThermalDomain's word for "whichever operator covers it"): a hex-8 brick as True; a hex-27 brick gets the
        # Hex27ElasticityBrickOperator, whose residual() is K_nonlinear_func (matrix_free = True keeps falling back on one); a slab falls back.
        if isinstance(matrix_free, str) and matrix_free != "any":
            raise ValueError("matrix_free: False, True or 'any'")
        self.hex27 = matrix_free == "any" and brick.itp_order == 2
        # matrix_free = True: no matrix at all.  self.A is the elasticity BrickOperator, K_linear = K_total = None, brick.pattern is never called and
        # K_linear_func only re-sends the parameters.  A brick the operator does not cover is built as the default domain is, and
        # matrix_free_reason says why (ThermalDomain's rule).
        self.matrix_free_reason = (brick_operator_elasticity_hex27_refusal(brick) if self.hex27 else brick_operator_refusal(brick)) if matrix_free else None
        self.matrix_free = bool(matrix_free) and self.matrix_free_reason is None
        if self.matrix_free:
            try:
                self.A = brick.elasticity_operator_hex27(lam, mu, tau, penalty_faces, traction_faces, self.sig) if self.hex27 else \
                    brick.elasticity_operator(lam, mu, tau, penalty_faces)
            except BrickOperatorRefused as e:
                self.matrix_free, self.matrix_free_reason = False, str(e)
        if not self.matrix_free:
            self.A = brick.pattern(3)
        n = self.A.n
        self.basicfield_size = n
        self.x = torch.zeros(n, dtype=torch.float64, device=dev)
        self.dx = torch.zeros(n, dtype=torch.float64, device=dev)
        self.x_star = torch.zeros(n, dtype=torch.float64, device=dev)
        self.residue = torch.zeros(n, dtype=torch.float64, device=dev)
        self.K_linear = None if self.matrix_free else torch.zeros(self.A.nnz, dtype=torch.float64, device=dev)
        self.K_total = self.K_linear  # a linear form: K_total .= K_linear is an alias
        self.converge_tol = 1e-6
        self.linear_solver: Callable = lambda gf: iterative_Solve(gf.A, gf.K_total, gf.residue, gf.converge_tol,
                                                                   Sv_func=idrs_, maxiter=2000, max_pass=10, s=8)[0]
        # multigrid = True (with matrix_free, tau != 0 on a penalty face): a hierarchy is attached to the operator and linear_solver is cg_ with the
        # V-cycle as its preconditioner.  On a domain that fell back to the assembled path, or without a penalty face (K is singular), the default
        # solver stays and multigrid_reason says why (ThermalDomain's rule).
        self.multigrid, self.multigrid_reason = False, None
        if multigrid:
            if not self.matrix_free:
                self.multigrid_reason = "the domain holds an assembled matrix (" + (self.matrix_free_reason or "matrix_free was not asked for") + \
                                        "): the multigrid preconditioner needs the matrix-free hex-8 operator"
            elif self.hex27:
                self.multigrid_reason = "a hex-27 elasticity operator: a multigrid hierarchy for it does not exist yet"
            elif tau == 0.0 or (penalty_faces & ALL_FACES) == 0:
                self.multigrid_reason = "no penalty face (tau == 0 or penalty_faces == 0): K keeps the rigid-body modes, the multigrid " \
                                        "preconditioner needs a definite K"
            else:
                self.multigrid = True
                self.mg = self.A.multigrid()  # (the solves run its setup: K_linear_func's parameters can never leave a stale level)
                self.linear_solver = lambda gf: iterative_Solve(gf.A, None, gf.residue, gf.converge_tol, Sv_func=cg_, Pr_func=Pr_Multigrid_,
                                                                maxiter=400, max_pass=4)[0]
        self.history = []

    def K_linear_func(self):
        if self.matrix_free:  # nothing is assembled: the parameters go to the operator
            if self.hex27:
                self.A.set_params(self.lam, self.mu, self.tau, self.penalty_faces, self.traction_faces, self.sig)
            else:
                self.A.set_params(self.lam, self.mu, self.tau, self.penalty_faces)
            return
        self.brick.assemble_elasticity(self.A, self.lam, self.mu, self.tau, self.penalty_faces, out=self.K_linear)

    def K_nonlinear_func(self):
        if self.matrix_free and self.hex27:  # (the fused residual kernels are hex-8: the operator's own residual)
            self.A.residual(self.x_star, out=self.residue)
            return
        self.brick.residual_elasticity(self.x_star, self.lam, self.mu, self.tau, self.penalty_faces, self.traction_faces, self.sig, out=self.residue)

    def update_OneStep(self, max_iter: int = 4):
        self.dx.zero_()
        self.K_linear_func()
        counter = -1
        self.history = []
        while True:
            torch.add(self.x, self.dx, out=self.x_star)
            self.K_nonlinear_func()
            res = normalized_norm(self.residue, self.brick.ctx)
            counter += 1
            self.history.append(res)
            if res < self.converge_tol or counter > max_iter:
                break
            delta_x = self.linear_solver(self)
            self.dx -= delta_x
        self.x += self.dx
        return self.history


@dataclass
class GeneralAlpha:
    """Static problems only here: max_time_level = 0, K_params = [1], beta = [1] (04_Time_Domain.jl:1-18)."""
    alpha_params: Tuple[float, ...] = (1.0, 1.0, 1.0)
    gamma_params: Tuple[float, ...] = (1.0, 1.0)


class ThermalDomain:
    """FEM_Domain + GlobalField for the thermal weak form of examples/thermal_conduction/3D_Script.jl:30-31
    on a structured brick: the two generated closures are the fused HIP kernels, update_OneStep is the
    reference's Newton driver (04_Time_Domain.jl:59-80)."""

    def __init__(self, brick: Brick, k: float, h: float, Tenv: float, robin_faces: int = ALL_FACES, *, fixed_faces: int = 0,
                 h_penalty: float = 0.0, Tw: float = 0.0, matrix_free=False, multigrid=False):
        self.brick, self.k, self.h, self.Tenv, self.robin_faces = brick, k, h, Tenv, robin_faces
        # weakly imposed Dirichlet faces (fix_boundary of examples/thermal_conduction/2D_Script.jl:58)
        self.fixed = dict(fixed_faces=fixed_faces, h_penalty=h_penalty, Tw=Tw)
        dev = f"cuda:{brick.ctx.device}"
        # matrix_free = True: no matrix at all.  self.A is a BrickOperator (K x and diag K straight from the coordinates), K_linear = K_total = None,
        # brick.pattern is never called and K_linear_func only re-sends the parameters; the default linear_solver hands (A, None) to iterative_Solve.
        # A brick the operator does not cover (brick_operator_refusal) is built as the default domain is: matrix_free is False then and
        # matrix_free_reason says why (GenericDomain's rule).
        # matrix_free = "any" (GenericDomain's word for "whichever operator covers it"): a hex-8 brick as True; a hex-27 brick gets the
        # Hex27BrickOperator (matrix_free = True keeps falling back on one); a slab falls back with the reason.
        if isinstance(matrix_free, str) and matrix_free != "any":
            raise ValueError("matrix_free: False, True or 'any'")
        hex27 = matrix_free == "any" and brick.itp_order == 2
        self.matrix_free_reason = (brick_operator_hex27_refusal(brick) if hex27 else brick_operator_refusal(brick)) if matrix_free else None
        self.matrix_free = bool(matrix_free) and self.matrix_free_reason is None
        if self.matrix_free:
            try:
                make = brick.thermal_operator_hex27 if hex27 else brick.thermal_operator
                self.A = make(k, h, Tenv, robin_faces, **self.fixed)
            except BrickOperatorRefused as e:  # (whatever rule the library applies beyond the host's forecast reaches the fallback too)
                self.matrix_free, self.matrix_free_reason = False, str(e)
        if not self.matrix_free:
            self.A = brick.pattern(1)  # assemble_Global_Variables! -> assemble_SparseID!
        n = self.A.n
        self.basicfield_size = n
        self.x = torch.zeros(n, dtype=torch.float64, device=dev)
        self.dx = torch.zeros(n, dtype=torch.float64, device=dev)
        self.x_star = torch.zeros(n, dtype=torch.float64, device=dev)
        self.residue = torch.zeros(n, dtype=torch.float64, device=dev)
        self.K_linear = None if self.matrix_free else torch.zeros(self.A.nnz, dtype=torch.float64, device=dev)
        self.K_total = self.K_linear  # no nonlinear gradients in this form: K_total .= K_linear is an alias
        self.s = torch.zeros(n, dtype=torch.float64, device=dev)  # controlpoints.s
        self.converge_tol = 1e-6
        self.linear_solver: Callable = lambda gf: iterative_Solve(gf.A, gf.K_total, gf.residue, gf.converge_tol,
                                                                   Sv_func=idrs_, maxiter=2000, max_pass=10, s=8)[0]
        # multigrid = True (with matrix_free, K symmetric): linear_solver is cg_ with the V-cycle as its preconditioner; on a hex-27 operator
        # (matrix_free = "any") the hierarchy is the p-coarsened one of Hex27BrickOperator.multigrid.  With fixed faces (K is nonsymmetric), on a
        # hex-27 brick with a rule below itg_order 4 or on a domain that fell back to the assembled path the default solver stays, and
        # multigrid_reason says why.  multigrid = "any": as True, and with fixed faces on a hex-8 brick gmres_ with the cycle of the nonsymmetric
        # hierarchy (BrickOperator.multigrid(nonsymmetric=True)).
        if isinstance(multigrid, str) and multigrid != "any":
            raise ValueError("multigrid: False, True or 'any'")
        self.multigrid, self.multigrid_reason = False, None
        if multigrid:
            if not self.matrix_free:
                self.multigrid_reason = "the domain holds an assembled matrix (" + (self.matrix_free_reason or "matrix_free was not asked for") + \
                                        "): the multigrid preconditioner needs a matrix-free brick operator"
            elif hex27 and brick.itg_order < 4:
                self.multigrid_reason = "a hex-27 brick with fewer than 3 Gauss points per direction (itg_order < 4): the under-integrated K keeps " \
                                        "near-null modes that the hex-8 coarse space of the multigrid preconditioner does not hold"
            elif fixed_faces and (h_penalty != 0.0 or k != 0.0) and multigrid == "any" and not hex27:
                # multigrid = "any": whichever solver takes the cycle -- with fixed faces on a hex-8 brick the nonsymmetric hierarchy and gmres_
                self.multigrid = True
                self.mg = self.A.multigrid(nonsymmetric=True)
                self.linear_solver = lambda gf: iterative_Solve(gf.A, None, gf.residue, gf.converge_tol, Sv_func=gmres_, Pr_func=Pr_Multigrid_,
                                                                maxiter=200, max_pass=4)[0]
            elif fixed_faces and (h_penalty != 0.0 or k != 0.0) and multigrid == "any":
                self.multigrid_reason = "fixed_faces make K nonsymmetric, and the nonsymmetric hierarchy that gmres_ takes covers the hex-8 thermal " \
                                        "operator only: not a hex-27 brick"
            elif fixed_faces and (h_penalty != 0.0 or k != 0.0):
                self.multigrid_reason = "fixed_faces make K nonsymmetric: the multigrid preconditioner needs cg_"
            else:
                self.multigrid = True
                self.mg = self.A.multigrid()  # (the solves run its setup: K_linear_func's parameters can never leave a stale level)
                self.linear_solver = lambda gf: iterative_Solve(gf.A, None, gf.residue, gf.converge_tol, Sv_func=cg_, Pr_func=Pr_Multigrid_,
                                                                maxiter=200, max_pass=4)[0]
        self.history = []

    def K_linear_func(self):
        if self.matrix_free:  # nothing is assembled: the parameters go to the operator
            self.A.set_params(self.k, self.h, self.Tenv, self.robin_faces, **self.fixed)
            return
        self.brick.assemble_thermal(self.A, self.k, self.h, self.Tenv, self.robin_faces, out=self.K_linear, **self.fixed)

    def K_nonlinear_func(self):
        self.brick.residual_thermal(self.x_star, self.k, self.h, self.Tenv, self.robin_faces, s=self.s, out=self.residue, **self.fixed)

    def update_OneStep(self, max_iter: int = 4):
        self.dx.zero_()  # initialize_dx! with max_time_level = 0
        self.K_linear_func()
        counter = -1
        self.history = []
        while True:
            torch.add(self.x, self.dx, out=self.x_star)  # update_x_star!
            self.K_nonlinear_func()
            res = normalized_norm(self.residue, self.brick.ctx)
            counter += 1
            self.history.append(res)
            if res < self.converge_tol or counter > max_iter:
                break
            delta_x = self.linear_solver(self)
            self.dx -= delta_x  # update_dx!(-delta_x), beta = 1
        self.x += self.dx
        return self.history
