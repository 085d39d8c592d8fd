"""The kernels over in-place tables (tpz_raw.hip) use no scratch (private segment) memory: the
view is a handful of registers computed from byte loads, and the walk reads the descriptors from
HBM field by field. Read from the built library as tests/test_scratch.py does; no GPU needed."""
import os

import pytest

from test_scratch import LIB, LLVM, kernel_scratch

RAW = ["raw_verify_kernel", "raw_seek_kernel", "raw_get_walk_kernel", "raw_lsm_get_walk_kernel",
       "raw_get_gather_kernel", "raw_lsm_get_gather_kernel"]


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="library not built / ROCm LLVM tools absent")
def test_raw_kernels_use_no_scratch(tmp_path):
    sizes = kernel_scratch(LIB, str(tmp_path))
    for pat in RAW:
        hits = {k: v for k, v in sizes.items() if pat + "E" in k}
        assert hits, f"{pat} not found in {sorted(sizes)}"
        assert all(v == 0 for v in hits.values()), hits
