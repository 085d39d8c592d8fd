"""The kernels of tpz_open.hip use no scratch (private segment) memory: the index walk's state is a
handful of registers, the staged tiles and the per-record positions live in LDS. Read from the built
library as tests/test_scratch.py does; no GPU needed."""
import os

import pytest

from test_scratch import LIB, LLVM, kernel_scratch

OPEN = ["open_index_kernel", "open_scan_kernel", "open_metas_kernel", "open_flags_kernel"]


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="library not built / ROCm LLVM tools absent")
def test_open_kernels_use_no_scratch(tmp_path):
    sizes = kernel_scratch(LIB, str(tmp_path))
    for pat in OPEN:
        hits = {k: v for k, v in sizes.items() if pat in k}
        assert hits, f"{pat} not found in {sorted(sizes)}"
        assert all(v == 0 for v in hits.values()), hits
