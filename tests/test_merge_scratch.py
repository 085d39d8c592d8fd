"""The merge's kernels (tpz_merge.hip) and tpz_flat_entry_pos use no scratch (private segment)
memory: the tile merge's items live in registers with static indices and in LDS, and the gather
moves bytes straight between the columns. Read from the built library as tests/test_scratch.py
does; no GPU needed."""
import os

import pytest

from test_scratch import LIB, LLVM, kernel_scratch

MERGE = ["merge_prefix_kernel", "merge_partition_kernel", "merge_tile_kernel", "merge_drop_kernel",
         "merge_gather_kernel", "flat_entry_pos_kernel"]


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="library not built / ROCm LLVM tools absent")
def test_merge_kernels_use_no_scratch(tmp_path):
    sizes = kernel_scratch(LIB, str(tmp_path))
    for pat in MERGE:
        hits = {k: v for k, v in sizes.items() if pat in k}
        assert hits, f"{pat} not found in {sorted(sizes)}"
        assert all(v == 0 for v in hits.values()), hits
