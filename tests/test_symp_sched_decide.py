"""CPU check of the patch sweep's schedule (csrc/symp_sched_decide.h), no GPU needed: tools/host_check_symp_sched.cpp, compiled with g++.

On the 512^3 geometry (64 x 16 patches, 509 swept planes, 3 runs per patch, 96 waves per XCD; flags by spc_expected's predicate), the 256^3 geometry and the
two fixtures of tests/test_gpu_symp_sched.py under their grid cap of 8, for the decision's own schedule, the identity schedule and two seeds of the
pseudo-random one: every run appears exactly once, a workgroup's runs lie in its XCD's patch range, the ranges are contiguous and cover all patches, the
table is the same when built twice, the identity schedule is the sweep's arithmetic form (equal shares, spc_run), the model makespan of the schedule is at
most the LPT bound (4/3 - 1/(3 W)) x max(mean load, costliest run) per XCD and, at 512^3, at most 0.83 of the identity schedule's and within a tenth of
perfect balance (0.75 was expected from a fitted cost of 1.4 us per flagged step; the per-run clocks measured 2.4 us, profiles/r13_symp_sched_ab_512.txt:
with whole runs of 830 or 408 us no assignment gets below 2.04 ms against the identity schedule's 2.48 ms); and the partial-sum rule:
512^3 unsplit fits per-run sums, 256^3 (3584 runs + 1792 workgroups) returns the per-workgroup form."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metafem.jl_amd", "csrc")


def test_host_check_symp_sched(tmp_path):
    exe = str(tmp_path / "host_check_symp_sched")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tools", "host_check_symp_sched.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-3000:]
    assert out.stdout.strip().endswith("OK")
