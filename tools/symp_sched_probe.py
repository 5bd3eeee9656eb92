"""Measure the cost constants of csrc/symp_sched_decide.h (SPS_CU_PS, SPS_CF_PS, SPS_CS0_PS) with a timestamp per run of the patch sweep.

Needs a PROBE BUILD of the library -- the sweep stamps wall_clock64() at every run's start and end only under -DSYMP_SCHED_CLOCKS, never in the shipped
library.  In a copy of the tree:
    make -C metafem.jl_amd/csrc CXXFLAGS='-O3 -std=c++17 -fPIC --offload-arch=gfx950 -DSYMP_SCHED_CLOCKS'
    python tools/symp_sched_probe.py [--n 512] [--out FILE]

hex-8 thermal brick of n^3 elements on the unit cube, a few Jacobi-CG iterations (cg_variant 4: the scaled copy the benchmark binds) under the identity
schedule (mode 1 of the "symp_sched" knob) and under the decision's own (mode 0).  The last product's stamps per run id come back; the flagged steps of a
run follow from the geometry (spc_expected's predicate).  Printed per mode: the least-squares fit  time = unflagged x CU + flagged x CF + CS0  over all
runs, the launch's span (first start to last end), the model makespan of the same lists with the fitted constants, and the workgroups that end last.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SP_L, SP_W = 4, 32
TICK_PS = 10000  # wall_clock64: 100 MHz


def spt_nseg(NP, slots, nplanes):
    best, best_eff = 1, 0.0
    for ns in range(1, min(max(nplanes // 16, 1), 64) + 1):
        R = NP * ns
        rounds = -(-R // slots)
        eff = R / (rounds * slots)
        if eff > best_eff + 1e-9:
            best_eff, best = eff, ns
        if eff >= 0.9:
            best = ns
            break
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    import metafem_jl_amd as mf
    from metafem_jl_amd import _lib

    fn = getattr(_lib.lib, "mfem_debug_symp_clocks", None)
    if fn is None:
        raise SystemExit("this library was not built with -DSYMP_SCHED_CLOCKS")
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], C.c_int
    n = args.n
    m = n + 1
    p0, p1 = 2, m - 2
    swept = (p1 - p0) * m * m
    B = 2 if swept >= 100000000 else 1
    L = SP_L * B
    ms1 = m - m % L if 1 <= m % L <= 1 else m
    ms2 = m - m % SP_W if 1 <= m % SP_W <= 2 else m
    NR, NPk = -(-ms1 // L), -(-ms2 // SP_W)
    NP, nplanes = NR * NPk, p1 - p0
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nseg = spt_nseg(NP, (7 if B == 1 else 3) * cus, nplanes)
    nruns = NP * nseg
    lines = [f"n = {n}: B = {B}, {NR} x {NPk} patches, {nplanes} swept planes, {nseg} runs per patch = {nruns} runs, {cus} CUs"]
    # the sweep stamps only where it keeps its sums per run (sps_per_run, csrc/symp_sched_decide.h): runs + workgroups within the 4096 partial sums
    grid = min(8 * -(-NP // 8) * nseg, ((7 if B == 1 else 3) * cus) & ~7)
    if nruns + grid > 4096:
        raise SystemExit(lines[0] + f": {nruns} runs + {grid} workgroups do not fit per-run sums; nothing would be stamped")
    # flagged / unflagged steps per run id = patch * nseg + seg
    flagged = np.zeros(nruns, dtype=np.int64)
    steps = np.zeros(nruns, dtype=np.int64)
    for patch in range(NP):
        j0, k0 = (patch // NPk) * L, (patch % NPk) * SP_W
        inner = j0 + L <= ms1 and j0 >= 2 and j0 + L - 1 <= m - 3 and k0 + SP_W <= ms2 and k0 >= 2 and k0 + SP_W - 1 <= m - 3
        for s in range(nseg):
            lo, hi = nplanes * s // nseg, nplanes * (s + 1) // nseg
            steps[patch * nseg + s] = hi - lo
            flagged[patch * nseg + s] = sum(1 for pl in range(lo, hi) if 2 <= p0 + pl <= m - 3) if inner else 0
    brick = mf.make_Brick((1.0, 1.0, 1.0), (n, n, n))
    A = brick.pattern(1)
    K = brick.assemble_thermal(A, 0.6, 25.0, 293.15, 0x3F)
    b = mf.FEM_rand(A.n, 11, 0) - 0.5
    buf = torch.zeros(4 * nruns, dtype=torch.int64, device="cuda")  # four words per run id; the sweep stamps run ids < nruns of a per-run launch only
    for mode in (1, 0):
        buf.zero_()
        _lib.check(fn(buf.data_ptr(), nruns))
        _lib.check(_lib.lib.mfem_debug_set(b"symp_sched", mode, 0))
        c0 = int(_lib.lib.mfem_debug_symp_const_count())
        mf.iterative_Solve(A, K, b, 1e-300, Sv_func=mf.cg_, Pr_func=mf.Pr_Jacobi_, maxiter=args.iters, max_pass=1, cg_variant=4, fixed_iterations=True)
        torch.cuda.synchronize()
        _lib.check(fn(None, 0))
        c = buf.cpu().numpy().reshape(-1, 4)[:nruns]
        if int(_lib.lib.mfem_debug_symp_const_count()) == c0 or not np.all(c[:, 1] > 0):
            lines.append(f"mode {mode}: the solve did not bind the constant form with per-run sums ({int((c[:, 1] > 0).sum())} of {nruns} runs stamped)")
            continue
        dur = (c[:, 1] - c[:, 0]).astype(np.float64) * TICK_PS
        # Where every run has the same number of steps to within one (512^3: 169 or 170) the start cost CS0 cannot be told from the per-step costs -- the
        # three columns are collinear -- and is left at zero: CU and CF then carry a run's start, spread over its steps.
        M = np.stack([(steps - flagged).astype(np.float64), flagged.astype(np.float64)], axis=1)
        with_start = steps.max() - steps.min() > 1
        if with_start:
            M = np.concatenate([M, np.ones((nruns, 1))], axis=1)
        sol = np.linalg.lstsq(M, dur, rcond=None)[0]
        cu, cf, cs0 = float(sol[0]), float(sol[1]), (float(sol[2]) if with_start else 0.0)
        fit = M @ sol
        for s in range(nseg):
            for name, sel in (("unflagged", (flagged == 0)), ("flagged", (flagged == steps))):
                pick = sel & (np.arange(nruns) % nseg == s)
                if pick.any():
                    lines.append(f"  mode {mode} segment {s}: {int(pick.sum())} wholly {name} runs of {int(steps[pick][0])} steps: mean {dur[pick].mean() * 1e-6:.1f} us "
                                 f"(min {dur[pick].min() * 1e-6:.1f}, max {dur[pick].max() * 1e-6:.1f})")
        span = (c[:, 1].max() - c[:, 0].min()) * TICK_PS
        wg = c[:, 2]
        load = np.zeros(int(wg.max()) + 1)
        np.add.at(load, wg, fit)
        busy = np.zeros_like(load)
        np.add.at(busy, wg, dur)
        end = np.zeros_like(load)
        np.maximum.at(end, wg, (c[:, 1] - c[:, 0].min()) * TICK_PS)
        lines.append(f"mode {mode}: CU = {cu:.0f} ps per unflagged step, CF = {cf:.0f} ps per flagged step, CS0 = {cs0:.0f} ps per run "
                     f"(rms residual {np.sqrt(np.mean((dur - fit) ** 2)) * 1e-6:.2f} us of mean {dur.mean() * 1e-6:.1f} us)")
        lines.append(f"  launch span {span * 1e-9:.4f} ms; model makespan with the fit {load.max() * 1e-9:.4f} ms; busiest workgroup {busy.max() * 1e-9:.4f} ms, "
                     f"mean {busy.mean() * 1e-9:.4f} ms; first start to a workgroup's last end: min {end.min() * 1e-9:.4f}, max {end.max() * 1e-9:.4f} ms")
        for w in np.argsort(-end)[:6]:
            mine = np.nonzero(wg == w)[0]
            mine = mine[np.argsort(c[mine, 3])]
            lines.append(f"  workgroup {int(w)} (XCD {int(w) % 8}) ends at {end[w] * 1e-9:.4f} ms: runs (patch, seg, unflagged, flagged, us) "
                         + ", ".join(f"({r // nseg}, {r % nseg}, {steps[r] - flagged[r]}, {flagged[r]}, {dur[r] * 1e-6:.0f})" for r in mine))
    _lib.lib.mfem_debug_set(b"symp_sched", 0, 0)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
