"""The kernels of tpz_tables.hip (tpz_entries_bound, tpz_table_cut, tpz_sst_finish) use no scratch
(private segment) memory: the finish kernels' per-thread arrays have static indices and stay in
registers. Read from the built library as tests/test_scratch.py does; no GPU needed."""
import os

import pytest

from test_scratch import LIB, LLVM, kernel_scratch

TABLES = ["entries_bound_kernel", "table_cut_kernel", "sst_klen_kernel", "sst_layout_kernel",
          "sst_meta_kernel", "sst_bloom_kernel", "sst_crc_kernel"]


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/clang-offload-bundler"),
                    reason="library not built / ROCm LLVM tools absent")
def test_tables_kernels_use_no_scratch(tmp_path):
    sizes = kernel_scratch(LIB, str(tmp_path))
    for pat in TABLES:
        hits = {k: v for k, v in sizes.items() if pat in k}
        assert hits, f"{pat} not found in {sorted(sizes)}"
        assert all(v == 0 for v in hits.values()), hits
