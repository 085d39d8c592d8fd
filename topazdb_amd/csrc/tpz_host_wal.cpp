// tpz_host_wal.cpp — host read side of the write-ahead log: tpz_wal_index, WalIterator's chain
// (src/wal/iterator.rs:34-45) over a WAL image in host memory as MemTable::open drives it
// (src/mem_table.rs:119-143). A record is BE u16 klen | key | BE u16 vlen | value (Entry::encode,
// src/block/builder.rs:72-81). Every record's start depends on the lengths of the one before it and
// the image carries no checksum, so the walk is serial and stays here, where the file arrives; the
// device takes over from the record starts (tpz_wal_entries, tpz_mem_build). Plain C++, no GPU.
#include <cstdint>

#include "../../include/tpz_gpu.h"

tpz_err tpz_wal_index(const uint8_t* h_image, uint64_t image_bytes, uint64_t* h_rec,
                      uint64_t rec_cap, uint64_t* h_info) {
  if (!h_info || (image_bytes && !h_image)) return TPZ_ERR_INVALID_ARG;
  uint64_t at = 0, n = 0;
  uint64_t how = TPZ_WAL_END_IMAGE;
  tpz_err rc = TPZ_SUCCESS;
  while (at < image_bytes) {                    // next(): `if self.data.is_empty()` (:35)
    const uint64_t left = image_bytes - at;
    bool ok = left >= 2;                        // get_u16 (:39)
    uint64_t klen = 0, vlen = 0;
    if (ok) {
      klen = ((uint64_t)h_image[at] << 8) | h_image[at + 1];
      ok = left - 2 >= klen && left - 2 - klen >= 2;        // data[..klen] (:40), get_u16 (:42)
    }
    if (ok) {
      vlen = ((uint64_t)h_image[at + 2 + klen] << 8) | h_image[at + 3 + klen];
      ok = left - 4 - klen >= vlen;                          // data[..vlen] (:43)
    }
    if (!ok) {
      how = TPZ_WAL_TRUNCATED;
      rc = TPZ_ERR_SIZES;
      break;
    }
    if (h_rec) {
      if (n + 1 >= rec_cap) return TPZ_ERR_NOMEM;            // room for this start and the end
      h_rec[n] = at;
    }
    n++;
    at += 4 + klen + vlen;
    if (klen == 0) {                            // is_valid() is false: open() stops (:125)
      how = TPZ_WAL_END_EMPTY_KEY;
      break;
    }
  }
  // (`at` is the end of the last whole record in every case: a truncated record does not move it)
  if (h_rec) {
    if (n >= rec_cap) return TPZ_ERR_NOMEM;
    h_rec[n] = at;
  }
  h_info[0] = n;
  h_info[1] = how;
  h_info[2] = at;
  h_info[3] = how == TPZ_WAL_TRUNCATED ? at : UINT64_MAX;
  return rc;
}
