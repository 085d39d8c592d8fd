"""The kernels over memtable runs (tpz_mem.hip, tpz_get.hip, tpz_scan.hip) use no scratch
(private segment) memory: the run descriptors are read from HBM field by field, as the walk reads the tables', and the gather moves
bytes straight between the columns. Read from the built library as tests/test_scratch.py does; no
GPU needed."""
import os

import pytest

from test_scratch import LIB, LLVM, kernel_scratch

MEM = ["mem_prefix_kernel", "lsm_get_walk_kernel", "lsm_get_gather_kernel", "lsm_scan_seek_kernel",
       "lsm_scan_merge_kernel", "lsm_scan_entries_kernel"]


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="library not built / ROCm LLVM tools absent")
def test_mem_kernels_use_no_scratch(tmp_path):
    sizes = kernel_scratch(LIB, str(tmp_path))
    for pat in MEM:
        hits = {k: v for k, v in sizes.items() if pat in k}
        assert hits, f"{pat} not found in {sorted(sizes)}"
        assert all(v == 0 for v in hits.values()), hits
