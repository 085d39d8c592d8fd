"""The get's kernels (tpz_get.hip) use no scratch (private segment) memory: the walk reads the
table descriptors from HBM field by field instead of copying them, and the gather moves bytes
straight between the columns. Read from the built library as tests/test_scratch.py does; no GPU
needed."""
import os

import pytest

from test_scratch import LIB, LLVM, kernel_scratch

GET = ["get_walk_kernel", "get_gather_kernel"]


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="library not built / ROCm LLVM tools absent")
def test_get_kernels_use_no_scratch(tmp_path):
    sizes = kernel_scratch(LIB, str(tmp_path))
    for pat in GET:
        hits = {k: v for k, v in sizes.items() if pat in k}
        assert hits, f"{pat} not found in {sorted(sizes)}"
        assert all(v == 0 for v in hits.values()), hits
