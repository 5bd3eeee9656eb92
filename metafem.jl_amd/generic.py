"""Generic (unstructured, any weak form) path of the MI355X backend: the host-side mirror of what
`compile_Updater_GPU` emits and `update_OneStep!` drives in the reference, executed with the C-ABI kernels.

  update_Mesh                         -> mfem_update_basic_elements / mfem_update_basic_boundary   (4_Update_Integrator.jl)
  assemble_Global_Variables!          -> mfem_pattern_build (+ vectors)                             (03_GlobalAssembly.jl:6-140)
  update_K_Linear_<id>                -> mfem_op_var (externals), coefficient broadcasts, mfem_op_kval   (05_CodeGenerator.jl:52-91)
  update_K_NonLinear_<id>             -> mfem_op_var, broadcasts, mfem_op_res, mfem_op_kval               (:93-154, 282-283)
  update_OneStep!                     -> Newton loop                                                  (04_Time_Domain.jl:59-80)

The coefficient expressions of a weak form (`vals = @. expr * K_params * w[:, ids]`, 05_CodeGenerator.jl:75,110,136)
are elementwise broadcasts over [itg, n_items] arrays; the reference evaluates them as Julia GPU broadcasts and so
does this mirror with torch elementwise ops on device tensors -- no kernel of the hot path is written in torch.
In the Julia integration those callables are the generated `@.` expressions.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .affine import AffineResidual, OperatorCoefficient, affine_residual, operator_coefficient  # noqa: F401  (the generalisations of constant_coefficient)


@dataclass
class ResTerm:
    dual_pos: int
    dual_s: int  # 0 value, 1 + d = d/dx_d
    fn: Callable


@dataclass
class GradTerm:
    dual_pos: int
    dual_s: int
    base_pos: int
    base_s: int
    fn: Callable
    td_order: int = 0


@dataclass
class WeakForm:
    """AssembleWeakform (02_LocalAssembly.jl:30-58): what the symbolic layer hands to the code generator."""
    inner_vars: List[Tuple[str, int, int, int]] = field(default_factory=list)  # (name, basic_pos, s, td_order)
    cp_ext_vars: List[Tuple[str, str, int]] = field(default_factory=list)  # (name, controlpoint symbol, s)
    normals: List[Tuple[str, int]] = field(default_factory=list)  # (name, component)
    residues: List[ResTerm] = field(default_factory=list)
    linear_gradients: List[GradTerm] = field(default_factory=list)
    nonlinear_gradients: List[GradTerm] = field(default_factory=list)

    def sparse_positions(self):
        return {(g.dual_pos, g.base_pos) for g in self.linear_gradients + self.nonlinear_gradients}


class _NeedsEnv(Exception):
    pass


class _NoEnv(dict):
    """Probe environment: a coefficient function that reads -- or merely asks about -- any inner variable / external / normal
    is not a constant (every way of looking into the mapping raises, including `'x' in env`, iteration and len)."""

    def _needs(self, *a, **k):
        raise _NeedsEnv(a[0] if a else "env")

    __getitem__ = get = __contains__ = __iter__ = __len__ = keys = values = items = setdefault = pop = _needs

    def __bool__(self):
        raise _NeedsEnv("env")


def constant_coefficient(fn) -> Optional[float]:
    """The value of a term's coefficient if it does not depend on the integration point, else None."""
    try:
        v = fn(_NoEnv())
    except _NeedsEnv:
        return None
    except Exception:
        return None
    if torch.is_tensor(v) or isinstance(v, np.ndarray):
        return None
    try:
        return float(v)
    except Exception:
        return None


def matrix_free_terms(domain_wf: "WeakForm", boundary_wfs: Sequence["WeakForm"], t: float = 0.0, dt: float = 1.0):
    """Eligibility of a problem for the matrix-free operator (GenericDomain(matrix_free=True)), decided on the host: no part has nonlinear
    gradients, and every linear gradient's coefficient is a constant or, on facets, a constant plus a linear function of the normal components,
    free of fields and externals (affine.operator_coefficient: probed, then checked numerically).
    -> (per part [(GradTerm, OperatorCoefficient)], None) or (None, the reason)."""
    parts = []
    for i, wf in enumerate([domain_wf] + list(boundary_wfs)):
        where = "the domain" if i == 0 else f"boundary group {i - 1}"
        if wf.nonlinear_gradients:
            return None, f"{where} has nonlinear gradient terms"
        terms = []
        for k, g in enumerate(wf.linear_gradients):
            c = operator_coefficient(g, wf, facet=i > 0, t=t, dt=dt)
            if c is None:
                return None, f"linear gradient {k} of {where}: its coefficient is not a constant" + (" plus a normal-linear part" if i else "")
            terms.append((g, c))
        parts.append(terms)
    return parts, None


@dataclass
class OperatorPart:
    """One part (the domain, or a boundary group) as GenericDomain(matrix_free="any") hands it to the operator."""
    constant: List[Tuple[GradTerm, OperatorCoefficient]]  # -> mfem_mesh_operator_set_terms, as matrix_free_terms analyses them
    variable_linear: List[GradTerm]  # linear gradients whose coefficient is not a constant (plus, on facets, a normal-linear part)
    nonlinear: List[GradTerm]

    @property
    def variable(self) -> List[GradTerm]:
        """The variable terms in slot order: the linear ones (filled by K_linear_func), then the nonlinear ones (K_nonlinear_func)."""
        return self.variable_linear + self.nonlinear


def matrix_free_parts(domain_wf: "WeakForm", boundary_wfs: Sequence["WeakForm"], t: float = 0.0, dt: float = 1.0) -> List[OperatorPart]:
    """The classifier of GenericDomain(matrix_free="any"), decided on the host: per part the constant terms (operator_coefficient, exactly as
    matrix_free_terms takes them) and the variable ones -- every nonlinear gradient and every linear gradient whose coefficient depends on fields,
    externals or, beyond the linear part, the normal.  Nothing is refused here: what is left to refuse are the library's caps."""
    parts = []
    for i, wf in enumerate([domain_wf] + list(boundary_wfs)):
        part = OperatorPart([], [], list(wf.nonlinear_gradients))
        for g in wf.linear_gradients:
            c = operator_coefficient(g, wf, facet=i > 0, t=t, dt=dt)
            if c is None:
                part.variable_linear.append(g)
            else:
                part.constant.append((g, c))
        parts.append(part)
    return parts


class _Group:
    """Integration hosts of one launch family (the elements, or the facets of one boundary group).  The geometry tables of the
    operator path (vals, weights, normals: update_BasicElements / update_BasicBoundary) are built by `build` on first access."""

    def __init__(self, build, host_ids, el_ids, itg, colour_offsets=None, facet_el=None, facet_eidx=None):
        self._build, self._tables = build, None
        self.host_ids, self.el_ids, self.itg = host_ids, el_ids, itg
        self.table_free = False  # set by GenericDomain(table_free=True); cleared for good when an entry point refuses this group
        self.colour_offsets = colour_offsets
        self.facet_el, self.facet_eidx = facet_el, facet_eidx  # boundary groups: element / local face id of every facet
        self.n = el_ids.numel()
        self.adj = None  # (adj_ptr, adj) of the fused residual, built on first use

    def tables(self):
        if self._tables is None:
            self._tables = self._build()
        return self._tables

    vals = property(lambda self: self.tables()[0])
    weights = property(lambda self: self.tables()[1])
    normals = property(lambda self: self.tables()[2])

    @property
    def table_bytes(self) -> int:
        return 0 if self._tables is None else sum(t.numel() * t.element_size() for t in self._tables if t is not None)


class _DirectPlan:
    """Handle of mfem_mesh_direct_plan_create; closed before its context (Context._children)."""

    def __init__(self, ctx, handle):
        self.ctx, self._h = ctx, handle
        ctx._children.add(self)

    def close(self):
        if self._h:
            lib.mfem_mesh_direct_plan_destroy(self._h)
            self._h = C.c_uint64()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GenericDomain:
    """FEM_Domain with one workpiece + GlobalField; static (max_time_level = 0) or generalised-alpha transient."""

    def __init__(self, ctx, space, coords: np.ndarray, cp_ids: np.ndarray, n_fields: int, domain_wf: WeakForm,
                 boundaries: Sequence[Tuple[np.ndarray, np.ndarray, WeakForm]],
                 element_colours: Optional[np.ndarray] = None, max_time_level: int = 0, dissipative: bool = True,
                 batched: bool = True, fused: bool = True, row_owner: bool = True, fused_residual: bool = False,
                 table_free: bool = False, direct_rows: bool = False, matrix_free=False):
        """coords [ncp, dim]; cp_ids [itp, nel] 0-based (controlpoint_IDs in basis order); boundaries =
        [(element_ID[nf], element_eindex[nf] 0-based local face ids, WeakForm)].  element_colours (optional):
        a colour per element such that same-colour elements share no control point -> atomics-free scatter with a fixed
        summation order; "auto" computes one with mesh.colour_Elements (elements and boundary facets); without it the
        operators use FP64 atomics like the reference (order of the additions, hence the last bits, not reproducible)."""
        self.ctx, self.space, self.n_fields = ctx, space, n_fields
        # batched = True: one mfem_op_*_batch launch per integration domain; False: one launch per term, the literal
        # call sequence of the reference's generated updaters (kept for parity tests of the single-term seam)
        self.batched = batched
        # fused = True: linear-gradient terms with constant coefficients go through mfem_mesh_assemble_elements / _facets
        # (geometry on the fly, all such terms of a domain in one launch); the other terms keep the operator path
        self.fused = fused
        # row_owner = True: the fused element assembly runs in its row-owner form (mfem_mesh_assemble_elements_rows: element
        # matrices -> scratch -> one wave per CSR row; no atomics, fixed summation order); False: scatter through the slot table
        self.row_owner = row_owner
        # fused_residual = True: residual terms affine in the fields and externals (affine.affine_residual) go through
        # mfem_mesh_residual_elements / _facets (geometry on the fly, one launch per integration domain); the other terms keep the
        # operator path, and the geometry tables it reads are built only if some group still needs them (table_bytes)
        self.fused_residual = fused_residual
        # table_free = True (implies fused and fused_residual): every other term -- the words of inner_vars and nodal externals, facet normals,
        # non-affine residual terms, variable-coefficient and nonlinear gradient terms -- goes through mfem_mesh_var_* / _res_* / _kval_*
        # (csrc/mesh_ops.hip: the S3 operators with geometry on the fly); no group builds its tables (table_bytes stays 0) unless an entry
        # point answers MFEM_ERR_UNSUPPORTED, after which that group alone takes the operator path
        self.table_free = table_free
        # direct_rows = True: where the fused element assembly would take its row-owner form, it takes the direct form instead
        # (mfem_mesh_assemble_elements_direct, csrc/mesh_direct.hip: the same rows in the same summation order, computed batch by batch from the
        # coordinates with NO element-matrix scratch); the plan is built on first use; on MFEM_ERR_UNSUPPORTED the two-pass form takes over for
        # this domain.  Facet groups and variable-coefficient terms are unchanged.
        self.direct_rows = direct_rows
        self._direct_plan = None
        # matrix_free = True (implies fused and fused_residual): no matrix at all.  self.A is a MeshOperator (mfem_mesh_operator_*: K x and diag K straight
        # from the mesh), K_linear / K_total / slots are None, assemble_SparseID is never called and K_linear_func only re-sends the terms (coefficient
        # times the current K_params); `linear_solver = lambda g: iterative_Solve(g.A, g.K_total, g.residue, ...)` works unchanged.  A problem that is
        # not eligible (matrix_free_terms) or that the library refuses (MFEM_ERR_UNSUPPORTED: the caps) is built as the default domain is:
        # matrix_free is False then and matrix_free_reason says why.
        # matrix_free = "any" (implies table_free): the same, for ANY weak form.  The constant terms go to the operator as above; every other gradient
        # term -- nonlinear, or linear with a field- or external-dependent coefficient (matrix_free_parts) -- is a VARIABLE term
        # (mfem_mesh_operator_set_variable_terms): per part one persistent buffer [n_var_terms, n_items, itg] of coefficients at the Gauss points,
        # registered once; K_linear_func fills the slices of the linear ones, K_nonlinear_func those of the nonlinear ones (_coef: the words of the
        # fields and externals evaluated without tables, in item order), and the operator reads them at every product.  No K_total, no _kval_*.
        # Falls back as above only when the library refuses (the caps) or the mesh is empty.
        if isinstance(matrix_free, str) and matrix_free != "any":
            raise ValueError("matrix_free: False, True or 'any'")
        self.matrix_free_any = matrix_free == "any"
        self.matrix_free, self.matrix_free_reason = bool(matrix_free), None
        self._var_buf: List[Optional[torch.Tensor]] = []
        if self.matrix_free_any:
            if cp_ids.shape[1] == 0:
                self.matrix_free, self.matrix_free_reason = False, "the mesh has no elements"
            self.table_free = table_free = True
            element_colours = None  # (no scatter anywhere on this path: the items keep their natural order, which is how the operator indexes vals)
        elif matrix_free:
            _, self.matrix_free_reason = matrix_free_terms(domain_wf, [b[2] for b in boundaries])
            self.matrix_free = self.matrix_free_reason is None
        if matrix_free:
            self.fused = self.fused_residual = fused = fused_residual = True
        if table_free:
            if not batched:
                raise ValueError("table_free=True needs batched=True: the single-term seam (mfem_op_var / _res / _kval) reads the stored tables")
            self.fused = self.fused_residual = fused = fused_residual = True
        self._affine_cache: Dict[Tuple[int, int], Tuple[Tuple[float, float], list]] = {}
        dev = f"cuda:{ctx.device}"
        self.dev = dev
        dim = space.dim
        itp, nel = cp_ids.shape
        ncp = coords.shape[0]
        self.ncp, self.nel, self.itp, self.dim = ncp, nel, itp, dim
        self.domain_wf = domain_wf
        self.bwfs = [b[2] for b in boundaries]
        f64 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
        i32 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.int32, device=dev)
        self.coords = f64(coords.T)  # SoA x1|x2|x3
        self.cp = i32(cp_ids.T + 1)  # (nel, itp) C order == [itp, nel] column-major, 1-based like the reference
        # ---- update_Mesh
        nsd = 1 + dim
        ref = f64(space.ref_itp_vals.ravel(order="F"))
        self._ref, self._itgw = ref, f64(space.itg_weight)
        # adjacency of the row-owner assembly: for every control point the (element * itp + local id) pairs, ascending
        flat = np.ascontiguousarray(cp_ids.T).ravel()
        self._adj = i32(np.argsort(flat, kind="stable"))
        self._adj_ptr = torch.tensor(np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=ncp))]), dtype=torch.int64, device=dev)

        def element_tables():
            vals = torch.empty(space.itg * itp * nsd * nel, dtype=torch.float64, device=dev)
            w = torch.empty(space.itg * nel, dtype=torch.float64, device=dev)
            check(lib.mfem_update_basic_elements(ctx._h, dim, space.itg, itp, nel, ncp, ref.data_ptr(), self._itgw.data_ptr(),
                                                 self.coords.data_ptr(), self.cp.data_ptr(), 1, vals.data_ptr(), w.data_ptr()))
            return vals, w, None
        auto_colours = isinstance(element_colours, str)
        if auto_colours:
            if element_colours != "auto":
                raise ValueError("element_colours: an array, None or 'auto'")
            from .mesh import colour_Elements

            element_colours = colour_Elements(cp_ids)
        if element_colours is not None:
            order = np.argsort(element_colours, kind="stable")
            offs = np.concatenate([[0], np.cumsum(np.bincount(element_colours, minlength=int(element_colours.max()) + 1))])
        else:
            order, offs = np.arange(nel), None
        ids = i32(order + 1)
        self.groups = [_Group(element_tables, ids, ids, space.itg, colour_offsets=offs)]
        nface = space.bdy_ref_itp_vals.shape[0]
        bref = f64(np.concatenate([space.bdy_ref_itp_vals[f].ravel(order="F") for f in range(nface)]))
        bw = f64(space.bdy_itg_weights.ravel())
        btan = f64(np.concatenate([space.bdy_tangent_directions[f].ravel(order="F") for f in range(nface)]))
        self._bref, self._bw, self._btan, self._nface = bref, bw, btan, nface
        for el, eidx, _ in boundaries:
            nf = len(el)
            eld, eid = i32(np.asarray(el) + 1), i32(np.asarray(eidx) + 1)

            def facet_tables(nf=nf, eld=eld, eid=eid):
                fv = torch.empty(space.itg_b * itp * nsd * nf, dtype=torch.float64, device=dev)
                fw = torch.empty(space.itg_b * nf, dtype=torch.float64, device=dev)
                fn = torch.empty(space.itg_b * dim * nf, dtype=torch.float64, device=dev)
                check(lib.mfem_update_basic_boundary(ctx._h, dim, space.itg_b, itp, nface, nf, ncp, bref.data_ptr(), bw.data_ptr(),
                                                     btan.data_ptr(), self.coords.data_ptr(), self.cp.data_ptr(), eld.data_ptr(),
                                                     eid.data_ptr(), 1, fv.data_ptr(), fw.data_ptr(), fn.data_ptr()))
                return fv, fw, fn.view(nf, dim, space.itg_b)
            if auto_colours and nf > 0:
                # boundary operators touch every node of the host element (05_CodeGenerator.jl:175-189): colour the facets
                # by their hosts' node sets (two facets of one element conflict automatically)
                fcol = colour_Elements(cp_ids[:, np.asarray(el)])
                forder = np.argsort(fcol, kind="stable")
                foffs = np.concatenate([[0], np.cumsum(np.bincount(fcol, minlength=int(fcol.max()) + 1))])
                host = i32(forder + 1)
                self.groups.append(_Group(facet_tables, host, i32(np.asarray(el)[forder] + 1), space.itg_b, colour_offsets=foffs,
                                          facet_el=eld, facet_eidx=eid))
                continue
            host = i32(np.arange(nf) + 1)
            self.groups.append(_Group(facet_tables, host, eld, space.itg_b, facet_el=eld, facet_eidx=eid))
        if not fused_residual:  # (the operator path reads the tables at every residual: built here, as they always were)
            for g in self.groups:
                g.tables()
        for g in self.groups:
            g.table_free = table_free
        # ---- assemble_Global_Variables!
        from . import assemble_SparseID  # late import: package root defines it

        self.variable_size = ncp
        self.basicfield_size = n_fields * ncp
        if self.matrix_free:
            self.A, self.slots = self._mesh_operator(), None
        if not self.matrix_free:
            self.A, self.slots = assemble_SparseID(self.cp, ncp, n_fields=n_fields, index_base=1, ctx=ctx)
        n = self.basicfield_size
        z = lambda m: torch.zeros(m, dtype=torch.float64, device=dev)
        # x, dx, x_star hold max_time_level + 1 blocks of basicfield_size (03_GlobalAssembly.jl:27-31)
        self.max_time_level = max_time_level
        nglob = (max_time_level + 1) * n
        self.x, self.dx, self.x_star, self.residue = z(nglob), z(nglob), z(nglob), z(n)
        self.K_linear = None if self.matrix_free else z(self.A.nnz)
        # K_total = K_linear + the nonlinear gradient terms (05_CodeGenerator.jl:282-283).  A form without nonlinear gradient terms never adds anything: its
        # K_total IS K_linear (the same storage, unless K_total_private asks for a copy a solver may scale in place) -- no second nnz-sized array (15 GB for hex-20
        # elasticity at 96^3), no copy per Newton step
        self._K_total_aliases = not any(wf.nonlinear_gradients for wf in [domain_wf] + [b[-1] for b in boundaries])
        self.K_total = self.K_linear if self._K_total_aliases or self.matrix_free else z(self.A.nnz)
        self.controlpoints: Dict[str, torch.Tensor] = {}
        self.converge_tol = 1e-6
        # GeneralAlpha (04_Time_Domain.jl:1-7); FEM_Domain builds it with dissipative = true (01_Types.jl:168)
        self.alpha_params = (1.0, 1.0, 1.0)
        self.gamma_params = (1.0, 1.0) if dissipative else (0.5, 0.5)
        self.beta_params = [1.0]
        self.K_params = [1.0]  # static: alpha_0 * beta_0 (04_Time_Domain.jl:13-17)
        self.t, self.dt = 0.0, 1.0
        self.linear_solver: Optional[Callable] = None
        # A linear_solver that writes into K_total -- iterative_Solve(..., scale_in_place=True) column-scales it (Pr_Jacobi!, 02_Preconditioner.jl:118)
        # -- needs K_total_private = True when K_total aliases K_linear: K_total then gets storage of its own, filled from K_linear at every Newton
        # iteration as the reference does (05_CodeGenerator.jl:282-283).  Otherwise the solve would scale K_linear itself and the next iteration of the
        # step would solve with the scaled matrix.  Off by default, so that solvers that only read K keep the memory of the alias.
        self.K_total_private = False
        self.history: List[float] = []

    # -- the matrix-free operator (matrix_free=True) -------------------------------------------------------------
    def _operator_terms(self, K_params):
        """Per part the ABI terms (dual_sd, base_sd, block, coef, normal coefficients) at the current t / dt, times K_params; None: not eligible."""
        if self.matrix_free_any:
            found = matrix_free_parts(self.domain_wf, self.bwfs, t=getattr(self, "t", 0.0), dt=getattr(self, "dt", 1.0))
            if getattr(self, "_op_parts", None) is not None and [len(p.constant) for p in found] != [len(p.constant) for p in self._op_parts]:
                self.matrix_free_reason = "a coefficient that was constant when the operator was built is not at this t / dt"
                return None
            parts, reason = [p.constant for p in found], None
        else:
            parts, reason = matrix_free_terms(self.domain_wf, self.bwfs, t=getattr(self, "t", 0.0), dt=getattr(self, "dt", 1.0))
        if parts is None:
            self.matrix_free_reason = reason
            return None
        return [[(g.dual_s, g.base_s, g.dual_pos * self.n_fields + g.base_pos, c.c0 * K_params[g.td_order],
                  tuple(v * K_params[g.td_order] for v in c.normal)) for g, c in terms] for terms in parts]

    def _mesh_operator(self):
        """The MeshOperator of this domain: the elements, then a part per boundary group that has linear gradients.  None (and matrix_free False,
        the reason set) when the library answers MFEM_ERR_UNSUPPORTED."""
        from . import MeshOperator

        parts = self._operator_terms([1.0] * 8)
        self._op_parts = matrix_free_parts(self.domain_wf, self.bwfs) if self.matrix_free_any else None
        nvar = [len(p.variable) for p in self._op_parts] if self.matrix_free_any else [0] * len(parts)
        op = MeshOperator(self.ctx, self.dim, self.itp, self.nel, self.ncp, self.n_fields, self.coords, self.cp, 1)
        self._op_part = [0] + [None] * len(self.bwfs)
        self._var_buf = [None] * len(parts)
        rc = op.set_elements(self.space.itg, self._ref, self._itgw, self._adj_ptr, self._adj, parts[0])
        for i, g in enumerate(self.groups[1:], start=1):
            if rc == -3 or not (parts[i] or nvar[i]) or g.facet_el.numel() == 0:
                continue
            ptr, adj = self._residual_adj(g)
            rc = op.add_facets(self.space.itg_b, self._nface, self._bref, self._bw, self._btan, g.facet_el, g.facet_eidx, ptr, adj, parts[i])
            self._op_part[i] = rc if rc >= 0 else None
        for i, g in enumerate(self.groups):  # the variable terms: one persistent buffer per part, registered once
            if rc == -3 or not nvar[i] or self._op_part[i] is None:
                continue
            buf = torch.zeros((nvar[i], g.n, g.itg), dtype=torch.float64, device=self.dev)
            rc = op.set_variable_terms(self._op_part[i], [(t.dual_s, t.base_s, t.dual_pos * self.n_fields + t.base_pos)
                                                          for t in self._op_parts[i].variable], buf)
            self._var_buf[i] = buf if rc == 0 else None
        if rc == -3:
            op.close()
            self.matrix_free, self.matrix_free_reason = False, "the library refused the operator: " + lib.mfem_last_error().decode()
            self._var_buf = []
            return None
        return op

    def _fill_variable(self, i: int, g: _Group, env: dict, nonlinear: bool):
        """Evaluates the coefficients of part i's variable linear (K_linear_func) or nonlinear (K_nonlinear_func) terms into their slices."""
        part = self._op_parts[i]
        terms, s0 = (part.nonlinear, len(part.variable_linear)) if nonlinear else (part.variable_linear, 0)
        for k, t in enumerate(terms):
            self._var_buf[i][s0 + k].copy_(self._coef(g, t.fn, env, self.K_params[t.td_order]))

    # -- assemble_X! / dessemble_X! (03_GlobalAssembly.jl:44-75)
    def assemble_X(self, infos):
        for sym, pos, td in infos:
            o = pos * self.ncp + td * self.basicfield_size
            self.x[o:o + self.ncp] = self.controlpoints[sym]

    def dessemble_X(self, infos):
        for sym, pos, td in infos:
            o = pos * self.ncp + td * self.basicfield_size
            self.controlpoints[sym] = self.x[o:o + self.ncp].clone()

    # -- operator wrappers ------------------------------------------------------------------------
    def _layout(self, g: _Group, colours: bool):
        offs = g.colour_offsets if colours else None
        if offs is None:
            return _lib.OpLayout(g.itg, self.itp, 1 + self.dim, g.weights.numel() // g.itg, 1, 0, None), None
        arr = (C.c_int64 * len(offs))(*[int(v) for v in offs])
        return _lib.OpLayout(g.itg, self.itp, 1 + self.dim, g.weights.numel() // g.itg, 1, len(offs) - 1, arr), arr

    def _var(self, g: _Group, s: int, shift: int, x: torch.Tensor) -> torch.Tensor:
        tgt = torch.zeros(g.n * g.itg, dtype=torch.float64, device=self.dev)  # FEM_buffer zeros (05_CodeGenerator.jl:4)
        L, _k = self._layout(g, False)
        check(lib.mfem_op_var(self.ctx._h, C.byref(L), g.vals.data_ptr(), s, shift, self.cp.data_ptr(), x.data_ptr(), tgt.data_ptr(),
                              g.host_ids.data_ptr(), g.el_ids.data_ptr(), g.n))
        return tgt.view(g.n, g.itg)

    def _w(self, g: _Group) -> torch.Tensor:
        """local_integral_weights[:, local_itg_hostIDs] as [n_items, itg]."""
        return g.weights.view(-1, g.itg)[(g.host_ids - 1).long()]

    def _kval(self, g: _Group, t: GradTerm, vals: torch.Tensor, K: torch.Tensor):
        u = t.dual_pos * self.n_fields + t.base_pos
        L, _k = self._layout(g, True)
        check(lib.mfem_op_kval(self.ctx._h, C.byref(L), g.vals.data_ptr(), t.dual_s, t.base_s, vals.data_ptr(),
                               self.slots[u].data_ptr(), 0, K.data_ptr(), g.host_ids.data_ptr(), g.el_ids.data_ptr(), g.n))

    def _res(self, g: _Group, t: ResTerm, vals: torch.Tensor):
        L, _k = self._layout(g, True)
        check(lib.mfem_op_res(self.ctx._h, C.byref(L), g.vals.data_ptr(), t.dual_s, vals.data_ptr(), t.dual_pos * self.ncp,
                              self.cp.data_ptr(), self.residue.data_ptr(), g.host_ids.data_ptr(), g.el_ids.data_ptr(), g.n))

    # -- batched operator wrappers (mfem_op_*_batch): all terms of one integration domain per launch ------------------
    def _var_many(self, g: _Group, words) -> List[torch.Tensor]:
        """words: [(sd, shift, x tensor)] -> list of [n_items, itg] tensors."""
        out: List[torch.Tensor] = []
        if g.table_free and words:
            got = self._var_free(g, words, None)
            if got is not None:
                return got
        L, _k = self._layout(g, False)
        for c0 in range(0, len(words), _lib.MAX_BATCH_TERMS):
            chunk = words[c0:c0 + _lib.MAX_BATCH_TERMS]
            tgt = torch.empty((len(chunk), g.n, g.itg), dtype=torch.float64, device=self.dev)
            terms = (_lib.VarBatchTerm * len(chunk))(*[_lib.VarBatchTerm(sd, 0, shift, x.data_ptr()) for sd, shift, x in chunk])
            check(lib.mfem_op_var_batch(self.ctx._h, C.byref(L), g.vals.data_ptr(), len(chunk), terms, self.cp.data_ptr(),
                                        tgt.data_ptr(), g.host_ids.data_ptr(), g.el_ids.data_ptr(), g.n))
            out += [tgt[i] for i in range(len(chunk))]
        return out

    def _kval_many(self, g: _Group, terms, env, w, K: torch.Tensor):
        """terms: GradTerms; coefficient tensors are evaluated here, stacked term-major, sorted by sparse block."""
        if not terms:
            return
        order = sorted(range(len(terms)), key=lambda i: terms[i].dual_pos * self.n_fields + terms[i].base_pos)
        if g.table_free:
            order = self._kval_free(g, terms, order, env, K)
            if not order:
                return
        if w is None:
            w = self._w(g)
        L, _k = self._layout(g, True)
        stride = self.nel * self.itp * self.itp
        for c0 in range(0, len(order), _lib.MAX_BATCH_TERMS):
            ids = order[c0:c0 + _lib.MAX_BATCH_TERMS]
            vals = torch.stack([self._vals(terms[i].fn, env, w, self.K_params[terms[i].td_order]) for i in ids])
            arr = (_lib.KvalTerm * len(ids))(*[_lib.KvalTerm(terms[i].dual_s, terms[i].base_s,
                                                             terms[i].dual_pos * self.n_fields + terms[i].base_pos, 0) for i in ids])
            check(lib.mfem_op_kval_batch(self.ctx._h, C.byref(L), g.vals.data_ptr(), len(ids), arr, vals.data_ptr(),
                                         self.slots.data_ptr(), stride, 0, K.data_ptr(), g.host_ids.data_ptr(),
                                         g.el_ids.data_ptr(), g.n))

    def _res_many(self, g: _Group, terms, env, w):
        if not terms:
            return
        order = sorted(range(len(terms)), key=lambda i: terms[i].dual_pos)
        if g.table_free:
            order = self._res_free(g, terms, order, env)
            if not order:
                return
        if w is None:
            w = self._w(g)
        L, _k = self._layout(g, True)
        for c0 in range(0, len(order), _lib.MAX_BATCH_TERMS):
            ids = order[c0:c0 + _lib.MAX_BATCH_TERMS]
            vals = torch.stack([self._vals(terms[i].fn, env, w) for i in ids])
            arr = (_lib.ResBatchTerm * len(ids))(*[_lib.ResBatchTerm(terms[i].dual_s, 0, terms[i].dual_pos * self.ncp) for i in ids])
            check(lib.mfem_op_res_batch(self.ctx._h, C.byref(L), g.vals.data_ptr(), len(ids), arr, vals.data_ptr(),
                                        self.cp.data_ptr(), self.residue.data_ptr(), g.host_ids.data_ptr(), g.el_ids.data_ptr(), g.n))

    def _externals(self, wf: WeakForm, g: _Group, env: dict):
        if g.table_free and (wf.cp_ext_vars or wf.normals):
            nrm = torch.empty((g.facet_el.numel(), self.dim, g.itg), dtype=torch.float64, device=self.dev) if wf.normals else None
            tg = self._var_free(g, [(s, 0, self.controlpoints[sym]) for _, sym, s in wf.cp_ext_vars], nrm)
            if tg is not None:
                for (name, _, _), t in zip(wf.cp_ext_vars, tg):
                    env[name] = t
                for name, comp in wf.normals:
                    env[name] = nrm[:, comp, :][(g.host_ids - 1).long()]
                env["t"], env["dt"] = self.t, self.dt
                return
        if self.batched and wf.cp_ext_vars:
            tg = self._var_many(g, [(s, 0, self.controlpoints[sym]) for _, sym, s in wf.cp_ext_vars])
            for (name, _, _), t in zip(wf.cp_ext_vars, tg):
                env[name] = t
        else:
            for name, sym, s in wf.cp_ext_vars:  # declare_Extervar_GPU (05_CodeGenerator.jl:15-50)
                env[name] = self._var(g, s, 0, self.controlpoints[sym])
        for name, comp in wf.normals:
            env[name] = g.normals[:, comp, :][(g.host_ids - 1).long()]
        env["t"], env["dt"] = self.t, self.dt

    def _vals(self, fn, env, w, scale=1.0) -> torch.Tensor:
        v = fn(env)
        if not torch.is_tensor(v):
            v = torch.full_like(w, float(v))
        return (v * scale * w).contiguous()

    # -- table-free operator wrappers (mfem_mesh_var_* / _res_* / _kval_*): the coefficient WITHOUT the weight, geometry on the fly ------
    def _refused(self, g: _Group, rc: int) -> bool:
        """MFEM_ERR_UNSUPPORTED from a table-free entry point: this group takes the operator path (and builds its tables) from now on."""
        if rc == -3:
            g.table_free = False
            return True
        check(rc)
        return False

    def _mesh_args(self, g: _Group):
        """The leading mesh arguments of the table-free entry points for this group."""
        h = self.ctx._h
        if g.facet_el is None:
            return (h, self.dim, self.space.itg, self.itp, self.nel, self.ncp, self._ref.data_ptr(), self._itgw.data_ptr(),
                    self.coords.data_ptr(), self.cp.data_ptr(), 1)
        return (h, self.dim, self.space.itg_b, self.itp, self._nface, g.facet_el.numel(), self.ncp, self._bref.data_ptr(), self._bw.data_ptr(),
                self._btan.data_ptr(), self.coords.data_ptr(), self.cp.data_ptr(), g.facet_el.data_ptr(), g.facet_eidx.data_ptr(), 1)

    def _coef(self, g: _Group, fn, env, scale=1.0) -> torch.Tensor:
        """The coefficient of a term as [n_items, itg], without the weight (a scalar is broadcast)."""
        v = fn(env)
        if not torch.is_tensor(v):
            return torch.full((g.n, g.itg), float(v) * scale, dtype=torch.float64, device=self.dev)
        v = (v * scale).to(torch.float64)
        return v.expand(g.n, g.itg).contiguous()

    def _var_free(self, g: _Group, words, normals) -> Optional[List[torch.Tensor]]:
        """_var_many without tables; normals (facets): the tensor [n_facets, dim, itg_b] to fill.  None: refused, nothing usable written."""
        out: List[torch.Tensor] = []
        chunks = [words[c0:c0 + _lib.MAX_BATCH_TERMS] for c0 in range(0, len(words), _lib.MAX_BATCH_TERMS)] or [[]]
        for k, chunk in enumerate(chunks):
            tgt = torch.empty((len(chunk), g.n, g.itg), dtype=torch.float64, device=self.dev)
            terms = (_lib.VarBatchTerm * max(len(chunk), 1))(*[_lib.VarBatchTerm(sd, 0, shift, x.data_ptr()) for sd, shift, x in chunk])
            if g.facet_el is None:
                rc = lib.mfem_mesh_var_elements(*self._mesh_args(g), len(chunk), terms, tgt.data_ptr(), g.host_ids.data_ptr(), g.n)
            else:
                nptr = normals.data_ptr() if normals is not None and k == 0 else None
                rc = lib.mfem_mesh_var_facets(*self._mesh_args(g), len(chunk), terms, tgt.data_ptr() if chunk else None, nptr,
                                              g.host_ids.data_ptr(), g.n)
            if self._refused(g, rc):
                return None
            out += [tgt[i] for i in range(len(chunk))]
        return out

    def _res_free(self, g: _Group, terms, order, env) -> list:
        """_res_many without tables; returns the term ids the operator path still has to add (empty unless refused)."""
        ptr, adj = self._residual_adj(g)
        fn = lib.mfem_mesh_res_elements if g.facet_el is None else lib.mfem_mesh_res_facets
        for c0 in range(0, len(order), _lib.MAX_BATCH_TERMS):
            ids = order[c0:c0 + _lib.MAX_BATCH_TERMS]
            vals = torch.stack([self._coef(g, terms[i].fn, env) for i in ids])
            arr = (_lib.ResBatchTerm * len(ids))(*[_lib.ResBatchTerm(terms[i].dual_s, 0, terms[i].dual_pos * self.ncp) for i in ids])
            rc = fn(*self._mesh_args(g), len(ids), arr, vals.data_ptr(), g.host_ids.data_ptr(), ptr.data_ptr(), adj.data_ptr(),
                    self.residue.data_ptr())
            if self._refused(g, rc):
                return order[c0:]
        return []

    def _kval_free(self, g: _Group, terms, order, env, K: torch.Tensor) -> list:
        """_kval_many without tables: the row-owner form on elements when the ranks exist, else the scatter form; returns the term ids left."""
        offs = g.colour_offsets
        ncol = 0 if offs is None else len(offs) - 1
        carr = None if offs is None else (C.c_int64 * len(offs))(*[int(v) for v in offs])
        stride = self.nel * self.itp * self.itp
        for c0 in range(0, len(order), _lib.MAX_BATCH_TERMS):
            ids = order[c0:c0 + _lib.MAX_BATCH_TERMS]
            vals = torch.stack([self._coef(g, terms[i].fn, env, self.K_params[terms[i].td_order]) for i in ids])
            arr = (_lib.KvalTerm * len(ids))(*[_lib.KvalTerm(terms[i].dual_s, terms[i].base_s,
                                                             terms[i].dual_pos * self.n_fields + terms[i].base_pos, 0) for i in ids])
            if g.facet_el is None and self.row_owner and self._row_ranks() is not None:
                rc = lib.mfem_mesh_kval_elements_rows(*self._mesh_args(g), len(ids), arr, vals.data_ptr(), g.host_ids.data_ptr(), self.n_fields,
                                                      self.A._h, self._adj_ptr.data_ptr(), self._adj.data_ptr(), self._ranks.data_ptr(),
                                                      K.data_ptr())
                if rc == 0:
                    continue
                if rc != -3:  # (MFEM_ERR_UNSUPPORTED: row too long / scratch too large -> the scatter form decides)
                    check(rc)
            fn = lib.mfem_mesh_kval_elements if g.facet_el is None else lib.mfem_mesh_kval_facets
            rc = fn(*self._mesh_args(g), len(ids), arr, vals.data_ptr(), self.slots.data_ptr(), stride, K.data_ptr(), g.host_ids.data_ptr(), g.n,
                    ncol, carr)
            if self._refused(g, rc):
                return order[c0:]
        return []

    def _parts(self):
        yield self.domain_wf, self.groups[0]
        for wf, g in zip(self.bwfs, self.groups[1:]):
            yield wf, g

    def _row_ranks(self) -> torch.Tensor:
        """Column ranks of the row-owner assembly (mfem_mesh_row_ranks), built on first use."""
        if getattr(self, "_ranks", None) is None:
            ranks = torch.empty(self.nel * self.itp * self.itp, dtype=torch.int16, device=self.dev)
            rc = lib.mfem_mesh_row_ranks(self.ctx._h, self.itp, self.nel, self.ncp, self.n_fields, self.A._h, self._adj_ptr.data_ptr(),
                                         self._adj.data_ptr(), self.cp.data_ptr(), 1, ranks.data_ptr())
            if rc == -3:  # MFEM_ERR_UNSUPPORTED: an element lists a control point twice -> the scatter form from now on
                self.row_owner = self.direct_rows = False  # (the direct form adds through the same ranks)
                return None
            check(rc)
            self._ranks = ranks
        return self._ranks

    def _direct(self):
        """The plan of the direct row assembly (mfem_mesh_direct_plan_create), built on first use; None once the form has been refused."""
        if self._direct_plan is None and self.direct_rows:
            if self.nel == 0 or self._row_ranks() is None:
                self.direct_rows = False
                return None
            h = C.c_uint64()
            rc = lib.mfem_mesh_direct_plan_create(self.ctx._h, self.itp, self.nel, self.ncp, self.n_fields, self.A._h, self._adj_ptr.data_ptr(),
                                                  self._adj.data_ptr(), self.cp.data_ptr(), 1, self._ranks.data_ptr(), C.byref(h))
            if rc == -3:  # MFEM_ERR_UNSUPPORTED: the two-pass form from now on
                self.direct_rows = False
                return None
            check(rc)
            self._direct_plan = _DirectPlan(self.ctx, h)
        return self._direct_plan if self.direct_rows else None

    def direct_stats(self) -> Optional[dict]:
        """mfem_mesh_direct_plan_stats of the plan in use (None without one)."""
        if self._direct_plan is None:
            return None
        st = _lib.MeshDirectStats()
        check(lib.mfem_mesh_direct_plan_stats(self._direct_plan._h, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in st._fields_}

    def _assemble_const(self, g: _Group, cterms, K: torch.Tensor):
        """cterms: [(GradTerm, coefficient)] -> one fused launch per colour (mfem_mesh_assemble_elements / _facets)."""
        cterms = sorted(cterms, key=lambda tc: tc[0].dual_pos * self.n_fields + tc[0].base_pos)
        offs = g.colour_offsets
        ncol = 0 if offs is None else len(offs) - 1
        carr = None if offs is None else (C.c_int64 * len(offs))(*[int(v) for v in offs])
        stride = self.nel * self.itp * self.itp
        for c0 in range(0, len(cterms), _lib.MAX_BATCH_TERMS):
            chunk = cterms[c0:c0 + _lib.MAX_BATCH_TERMS]
            arr = (_lib.ConstTerm * len(chunk))(*[_lib.ConstTerm(t.dual_s, t.base_s, t.dual_pos * self.n_fields + t.base_pos, 0,
                                                                 c * self.K_params[t.td_order]) for t, c in chunk])
            if g.facet_el is None and self.row_owner and self._row_ranks() is not None:
                fresh = getattr(self, "_K_fresh", False) and K is self.K_linear and self.nel > 0
                plan = self._direct()
                if plan is not None:
                    rc = lib.mfem_mesh_assemble_elements_direct(self.ctx._h, self.dim, self.space.itg, self.itp, self.nel, self.ncp,
                                                                self._ref.data_ptr(), self._itgw.data_ptr(), self.coords.data_ptr(),
                                                                self.cp.data_ptr(), 1, len(chunk), arr, self.n_fields, self.A._h, plan._h,
                                                                K.data_ptr(), 1 if fresh else 0)
                    if rc == 0:
                        if fresh:
                            self._K_fresh = False
                        continue
                    if rc != -3:
                        check(rc)
                    self.direct_rows = False  # MFEM_ERR_UNSUPPORTED (the element's tables leave no LDS for the rows): the two-pass form for this domain
                fn = lib.mfem_mesh_assemble_elements_rows_set if fresh else lib.mfem_mesh_assemble_elements_rows
                rc = fn(self.ctx._h, self.dim, self.space.itg, self.itp, self.nel, self.ncp,
                                                          self._ref.data_ptr(), self._itgw.data_ptr(), self.coords.data_ptr(),
                                                          self.cp.data_ptr(), 1, len(chunk), arr, self.n_fields, self.A._h,
                                                          self._adj_ptr.data_ptr(), self._adj.data_ptr(), self._row_ranks().data_ptr(),
                                                          K.data_ptr())
                if rc == 0:
                    if fresh:
                        self._K_fresh = False
                    continue
                if rc != -3:  # MFEM_ERR_UNSUPPORTED (row too long / scratch too large) falls back to the scatter form
                    check(rc)
            self._K_started(K)
            if g.facet_el is None:
                check(lib.mfem_mesh_assemble_elements(self.ctx._h, self.dim, self.space.itg, self.itp, self.nel, self.ncp,
                                                      self._ref.data_ptr(), self._itgw.data_ptr(), self.coords.data_ptr(),
                                                      self.cp.data_ptr(), 1, len(chunk), arr, self.slots.data_ptr(), stride,
                                                      K.data_ptr(), g.host_ids.data_ptr(), g.n, ncol, carr))
            else:
                check(lib.mfem_mesh_assemble_facets(self.ctx._h, self.dim, self.space.itg_b, self.itp, self._nface,
                                                    g.facet_el.numel(), self.ncp, self._bref.data_ptr(), self._bw.data_ptr(),
                                                    self._btan.data_ptr(), self.coords.data_ptr(), self.cp.data_ptr(),
                                                    g.facet_el.data_ptr(), g.facet_eidx.data_ptr(), 1, len(chunk), arr,
                                                    self.slots.data_ptr(), stride, K.data_ptr(), g.host_ids.data_ptr(), g.n, ncol,
                                                    carr))

    # -- generated updater bodies -------------------------------------------------------------------
    def K_linear_func(self):
        # K_linear starts from zero (05_CodeGenerator.jl:282).  When the first thing it receives is the row-owner element assembly, that launch WRITES
        # every row instead (mfem_mesh_assemble_elements_rows_set): no memset, no read of the zeros.
        if self.matrix_free:  # nothing is assembled: the terms, times this step's K_params, go to the operator
            parts = self._operator_terms(self.K_params)
            if parts is None:
                raise _lib.MetaFEMError("matrix_free: " + self.matrix_free_reason)
            for terms, part in zip(parts, self._op_part):
                if part is not None and self.A.set_terms(part, terms) == -3:
                    raise _lib.MetaFEMError("matrix_free: " + lib.mfem_last_error().decode())
            for i, (wf, g) in enumerate(self._parts()):  # (matrix_free="any": the variable linear gradients -> their slices of the part's buffer)
                if i < len(self._var_buf) and self._var_buf[i] is not None and self._op_parts[i].variable_linear:
                    env = {}
                    self._externals(wf, g, env)
                    self._fill_variable(i, g, env, nonlinear=False)
            return
        self._K_fresh = True
        for wf, g in self._parts():
            if not wf.linear_gradients:
                continue
            terms = wf.linear_gradients
            if self.fused:
                coefs = [constant_coefficient(t.fn) for t in terms]
                cterms = [(t, c) for t, c in zip(terms, coefs) if c is not None]
                terms = [t for t, c in zip(terms, coefs) if c is None]
                if cterms:
                    self._assemble_const(g, cterms, self.K_linear)
                if not terms:
                    continue
            self._K_started(self.K_linear)
            env: dict = {}
            self._externals(wf, g, env)
            if self.batched:
                self._kval_many(g, terms, env, None if g.table_free else self._w(g), self.K_linear)
                continue
            w = self._w(g)
            for t in terms:
                self._kval(g, t, self._vals(t.fn, env, w, self.K_params[t.td_order]), self.K_linear)
        self._K_started(self.K_linear)

    def _K_started(self, K: torch.Tensor):
        """Zero K unless something has been put into it since K_linear_func began."""
        if getattr(self, "_K_fresh", False):
            K.zero_()
            self._K_fresh = False

    @property
    def table_bytes(self) -> int:
        """Bytes of geometry tables (vals, weights, normals of every group) currently allocated."""
        return sum(g.table_bytes for g in self.groups)

    def _affine_terms(self, i: int, wf: WeakForm):
        """[AffineResidual or None] per residual term of part i, for the current t / dt (re-analysed when they change)."""
        key = (float(self.t), float(self.dt))
        hit = self._affine_cache.get(i)
        if hit is None or hit[0] != key:
            from .affine import affine_residual

            hit = (key, [affine_residual(t, wf, t=key[0], dt=key[1]) for t in wf.residues])
            self._affine_cache[i] = hit
        return hit[1]

    def _residual_adj(self, g: _Group):
        if g.facet_el is None:
            return self._adj_ptr, self._adj
        if g.adj is None:  # facets: (facet * itp + local node) per control point of the host elements, ascending
            flat = (self.cp[(g.facet_el - 1).long()] - 1).reshape(-1).long()
            adj = torch.sort(flat, stable=True)[1].to(torch.int32)
            ptr = torch.zeros(self.ncp + 1, dtype=torch.int64, device=self.dev)
            ptr[1:] = torch.cumsum(torch.bincount(flat, minlength=self.ncp), 0)
            g.adj = (ptr, adj)
        return g.adj

    def _residual_fused(self, g: _Group, descs) -> bool:
        """One fused residual launch for the affine terms of a group; False (nothing added) if they exceed the caps."""
        from .affine import CapsExceeded, pack_affine

        def source(k):
            if k[0] == "x":
                _, pos, td, word = k
                return word, td * self.basicfield_size + pos * self.ncp, self.x_star.data_ptr()
            x = self.controlpoints[k[1]]
            if x.dtype != torch.float64 or not x.is_contiguous() or x.numel() < self.ncp or x.device != self.x_star.device:
                raise CapsExceeded(f"external {k[1]!r}: not a contiguous float64 device array of ncp entries")
            return k[2], 0, x.data_ptr()

        try:
            syms, nsym, terms, nterm, _ = pack_affine(descs, source)
        except CapsExceeded:
            return False
        ptr, adj = self._residual_adj(g)
        if g.facet_el is None:
            rc = lib.mfem_mesh_residual_elements(self.ctx._h, self.dim, self.space.itg, self.itp, self.nel, self.ncp, self._ref.data_ptr(),
                                                 self._itgw.data_ptr(), self.coords.data_ptr(), self.cp.data_ptr(), 1, nsym, syms, nterm,
                                                 terms, ptr.data_ptr(), adj.data_ptr(), self.residue.data_ptr())
        else:
            rc = lib.mfem_mesh_residual_facets(self.ctx._h, self.dim, self.space.itg_b, self.itp, self._nface, g.facet_el.numel(), self.ncp,
                                               self._bref.data_ptr(), self._bw.data_ptr(), self._btan.data_ptr(), self.coords.data_ptr(),
                                               self.cp.data_ptr(), g.facet_el.data_ptr(), g.facet_eidx.data_ptr(), 1, nsym, syms, nterm,
                                               terms, ptr.data_ptr(), adj.data_ptr(), self.residue.data_ptr())
        if rc == -3:  # MFEM_ERR_UNSUPPORTED (caps, LDS): the operator path takes these terms
            return False
        check(rc)
        return True

    def K_nonlinear_func(self):
        self.residue.zero_()
        if not self.matrix_free:  # (matrix_free: no K_total, the operator is the matrix)
            if self.K_total_private and self.K_total is self.K_linear:
                self.K_total = torch.empty_like(self.K_linear)
            if self.K_total is not self.K_linear:
                self.K_total.copy_(self.K_linear)  # 05_CodeGenerator.jl:282-283
        for i, (wf, g) in enumerate(self._parts()):
            residues = wf.residues
            if self.fused_residual and not residues and not wf.nonlinear_gradients:
                continue  # (nothing to add: the operator path would only build the tables)
            if self.fused_residual and residues:
                descs = self._affine_terms(i, wf)
                aff = [d for d in descs if d is not None]
                if aff and self._residual_fused(g, aff):
                    residues = [t for t, d in zip(wf.residues, descs) if d is None]
                if not residues and not wf.nonlinear_gradients:
                    continue
            env: dict = {}
            if self.batched:
                tg = self._var_many(g, [(s, td * self.basicfield_size + pos * self.ncp, self.x_star) for _, pos, s, td in wf.inner_vars])
                for (name, _, _, _), t in zip(wf.inner_vars, tg):
                    env[name] = t
                self._externals(wf, g, env)
                w = None if g.table_free else self._w(g)  # (table-free: the kernels multiply the weight in)
                self._res_many(g, residues, env, w)
                if self.matrix_free_any and self.matrix_free:  # (the tangent is the operator: the coefficients go straight to its buffer)
                    if self._var_buf[i] is not None:
                        self._fill_variable(i, g, env, nonlinear=True)
                    continue
                self._kval_many(g, wf.nonlinear_gradients, env, w, self.K_total)
                continue
            for name, pos, s, td in wf.inner_vars:  # declare_Innervar_GPU (:1-13)
                env[name] = self._var(g, s, td * self.basicfield_size + pos * self.ncp, self.x_star)
            self._externals(wf, g, env)
            w = self._w(g)
            for t in residues:
                self._res(g, t, self._vals(t.fn, env, w))
            for t in wf.nonlinear_gradients:
                self._kval(g, t, self._vals(t.fn, env, w, self.K_params[t.td_order]), self.K_total)

    # -- time domain (04_Time_Domain.jl:9-49) ---------------------------------------------------------
    def update_Time(self):
        L = self.max_time_level
        self.t += self.dt
        prod_gamma = [float(np.prod(self.gamma_params[:i])) for i in range(L + 1)]
        self.beta_params = [1.0 / (prod_gamma[i] * self.dt ** i) for i in range(L + 1)]
        self.K_params = [self.alpha_params[i] * self.beta_params[i] for i in range(L + 1)]

    def _level(self, v: torch.Tensor, lvl: int) -> torch.Tensor:
        n = self.basicfield_size
        return v[lvl * n:(lvl + 1) * n]

    def initialize_dx(self):
        self.dx.zero_()
        for lvl in range(self.max_time_level, 0, -1):  # predictor: dx[l-1] = dt (x[l] + gamma_l dx[l])
            torch.add(self._level(self.x, lvl), self._level(self.dx, lvl), alpha=self.gamma_params[lvl - 1],
                      out=self._level(self.dx, lvl - 1))
            self._level(self.dx, lvl - 1).mul_(self.dt)

    def update_dx(self, delta_x: torch.Tensor):
        for lvl in range(self.max_time_level + 1):
            self._level(self.dx, lvl).add_(delta_x, alpha=self.beta_params[lvl])

    def update_x_star(self):
        for lvl in range(self.max_time_level + 1):
            torch.add(self._level(self.x, lvl), self._level(self.dx, lvl), alpha=self.alpha_params[lvl],
                      out=self._level(self.x_star, lvl))

    def update_OneStep(self, max_iter: int = 4):
        """update_OneStep! (04_Time_Domain.jl:59-80)."""
        from . import normalized_norm

        self.update_Time()
        self.initialize_dx()
        self.K_linear_func()
        counter = -1
        self.history = []
        while True:
            self.update_x_star()
            self.K_nonlinear_func()
            res = normalized_norm(self.residue, self.ctx)
            counter += 1
            self.history.append(res)
            if res < self.converge_tol or counter > max_iter:
                break
            delta_x = self.linear_solver(self)
            self.update_dx(-delta_x)
        self.x += self.dx
        return self.history
