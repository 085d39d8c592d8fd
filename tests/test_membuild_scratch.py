"""The kernels of tpz_mem_build and tpz_wal_entries (tpz_membuild.hip) use no scratch (private
segment) memory. Read from the built library as tests/test_scratch.py does; no GPU needed."""
import os

import pytest

from test_scratch import LIB, LLVM, kernel_scratch

BUILD = ["mb_tile_sort_kernel", "mb_partition_kernel", "mb_tile_merge_kernel", "mb_pick_kernel",
         "mb_gather_kernel", "wal_len_kernel", "wal_copy_kernel"]


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="library not built / ROCm LLVM tools absent")
def test_membuild_kernels_use_no_scratch(tmp_path):
    sizes = kernel_scratch(LIB, str(tmp_path))
    for pat in BUILD:
        hits = {k: v for k, v in sizes.items() if pat in k}
        assert hits, f"{pat} not found in {sorted(sizes)}"
        assert all(v == 0 for v in hits.values()), hits
