"""The code paths the product library selects by environment variable: TPZ_BLOOM_ATOMIC (the
atomic bloom kernel for every filter), TPZ_BLOOM_GATHER (the staged gather build),
TPZ_PLAN_BISECT (the block plan's next-entry search without its guess) and TPZ_PLAN_GLOBAL_WALK
(the plan's table and walk in global memory). Each is read once into a `static const bool`, so
each case runs in a fresh child process with that one variable set; the child runs the parity
cases of the bloom and write-side tests and prints one line.
"""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "topazdb_amd", "csrc")
VARS = {"TPZ_BLOOM_ATOMIC": "tpz_api.cpp", "TPZ_BLOOM_GATHER": "tpz_seek.hip",
        "TPZ_PLAN_BISECT": "tpz_encode.hip", "TPZ_PLAN_GLOBAL_WALK": "tpz_encode.hip"}


def bloom_cases(ctx) -> int:
    """The bloom parity cases a child runs: 6 slices, 275 slices (tests/test_gpu_bloom_slices.py),
    the largest filter of tests/test_gpu_encode.py's test and the keys of every length up to
    65,535 bytes (tests/test_gpu_xxh3_lengths.py). Returns how many ran."""
    from test_gpu_bloom_slices import TINY, build_and_compare, reach
    from test_gpu_encode import test_device_bloom_build
    from test_gpu_xxh3_lengths import long_key_bloom_case
    assert reach(2000, TINY)[:2] == (6, 3) and reach(100_000, TINY)[:2] == (275, 123)
    build_and_compare(ctx, 2000, TINY)
    build_and_compare(ctx, 100_000, TINY)
    test_device_bloom_build(ctx, 60000, 0.001, 24)
    long_key_bloom_case(ctx)
    return 4


def plan_cases(ctx) -> int:
    """Three rows of test_async_plan_and_encode (block sizes 64, 4096 and 65536) against the
    oracle's builder. Returns how many ran."""
    from test_gpu_encode import test_async_plan_and_encode
    rows = [(64, 8, 20, 3000), (4096, 40, 400, 5000), (65536, 200, 3000, 3000)]
    for row in rows:
        test_async_plan_and_encode(ctx, *row)
    return len(rows)


CHILD = r"""
import os, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import torch
from topazdb_amd import _lib
import test_gpu_env_paths as E
assert os.environ.get({var!r}) == "1" and E.others_unset({var!r})
assert torch.cuda.is_available()
ctx = _lib.Context(0)
n = E.{cases}(ctx)
ctx.close()
print("ENV-PATH", {var!r}, "cases", n, "OK")
"""


def others_unset(var: str) -> bool:
    return not any(v in os.environ for v in VARS if v != var)


@pytest.mark.parametrize("var,cases", [("TPZ_BLOOM_ATOMIC", "bloom_cases"),
                                       ("TPZ_BLOOM_GATHER", "bloom_cases"),
                                       ("TPZ_PLAN_BISECT", "plan_cases"),
                                       ("TPZ_PLAN_GLOBAL_WALK", "plan_cases")])
def test_env_selected_path(var, cases):
    # the library still reads the variable (a renamed probe would leave this test on the default path)
    text = open(os.path.join(CSRC, VARS[var])).read()
    assert len(re.findall(r'static const bool \w+ = std::getenv\("%s"\) != nullptr' % var, text)) == 1
    env = {k: v for k, v in os.environ.items() if k not in VARS}
    env[var] = "1"
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), var=var, cases=cases)
    flags = ["-s"] if sys.flags.no_user_site else []      # the child sees the packages the parent sees
    r = subprocess.run([sys.executable, *flags, "-c", code], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("ENV-PATH")]
    assert lines == [f"ENV-PATH {var} cases {4 if cases == 'bloom_cases' else 3} OK"]
