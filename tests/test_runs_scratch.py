"""The kernels of tpz_runs.hip use no scratch (private segment) memory: the run table is read where
it lies in the kernel arguments, and the diagnostic form's funnel shift picks its words with
selects on the uniform shift and its byte-granular pieces select bytes without indexing a register
array. Read from the built library as tests/test_scratch.py does; no GPU needed."""
import os

import pytest

from test_scratch import LIB, LLVM, kernel_scratch

RUNS = ["runs_sizes_kernel", "runs_finish_kernel", "runs_gather_kernel"]


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="library not built / ROCm LLVM tools absent")
def test_runs_kernels_use_no_scratch(tmp_path):
    sizes = kernel_scratch(LIB, str(tmp_path))
    for pat in RUNS:
        hits = {k: v for k, v in sizes.items() if pat in k}
        assert hits, f"{pat} not found in {sorted(sizes)}"
        assert all(v == 0 for v in hits.values()), hits
    assert len([k for k in sizes if "runs_gather_kernel" in k]) == 2     # both forms of the gather
