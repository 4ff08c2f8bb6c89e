"""The pure planning helpers of DivideRounds' host scheduling (segment
bounds, transpose tile lists, the incremental resume round:
babble_amd/csrc/engine/sched_plan.h) against brute-force restatements, in
tests/cpp/sched_plan_check -- a plain g++ host program, no device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "sched_plan_check")


def test_sched_plan_check():
    subprocess.check_call(["make", "-s", "-C", ROOT, "tests/cpp/sched_plan_check"])
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "sched_plan ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
