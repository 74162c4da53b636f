// Host-side API of the CDNA4 kernel suite (pure HIP, gfx950).
// Implemented in kernels.hip, aggregate.hip and topk.hip; called from the torch
// binding (binding.cpp).
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

namespace hsk {

// K2: Spark-compatible Murmur3 fold over one column into h (u32 in u32 buf).
// kind: 0 = i32-hash (int32 input), 1 = i64-hash (int64 input), 2 = float32
// and 3 = float64 bits, hashed with -0.0 as +0.0 and every NaN as the
// canonical quiet NaN (Java floatToIntBits / doubleToLongBits).
// valid: optional per-row validity bytes — a null row leaves h unchanged
// (Spark Murmur3Hash skips null children); nullptr = all valid.
void murmur3_column(const void* vals, int kind, const uint8_t* valid,
                    uint32_t* h, int64_t n, bool first, uint32_t seed,
                    hipStream_t stream);
// The fold over the LAST key column with the pmod applied in the same
// kernel: out[i] = pmod(fold(h[i] or seed, vals[i]), num_buckets).  h is
// only read, and may be null when first (a single key column).
void murmur3_last_column(const void* vals, int kind, const uint8_t* valid,
                         const uint32_t* h, int32_t* out, int64_t n,
                         bool first, uint32_t seed, int32_t num_buckets,
                         hipStream_t stream);

// order-preserving u64 normalization (dtype codes: 0=i64,1=i32,2=f64,3=f32,
// 4=i16, 5=i8, 6=bool/u8).  canonical: float zeros and NaNs collapse first
// (SQL equality: the key of -0.0 is that of +0.0, all NaNs share the top key)
// descending: the bitwise complement of that key, so ascending u64 order of
// the result is descending order of the values (ORDER BY ... DESC).
void normalize_key(const void* vals, int dtype, uint64_t* out, int64_t n,
                   hipStream_t stream, bool canonical = false,
                   bool descending = false);
// d_mask[0] |= OR over i of (keys[i] ^ keys[0]): a superset of the key bits
// that vary.  d_mask must hold 0 (or bits to keep) on entry.
void key_varying_bits(const uint64_t* keys, int64_t n, uint64_t* d_mask,
                      hipStream_t stream);

// K3: stable LSD radix sort of (u64 key, i64 payload), ascending u64 order.
// keys/payload are sorted in place; tmp buffers same size provided by caller.
void radix_sort_pairs(uint64_t* keys, int64_t* payload, uint64_t* tmp_keys,
                      int64_t* tmp_payload, uint32_t* hist, uint64_t* d_mask,
                      int64_t n, hipStream_t stream);
void radix_sort_pairs32(uint64_t* keys, int32_t* payload,
                        uint64_t* tmp_keys, int32_t* tmp_payload,
                        uint32_t* hist, uint64_t* d_mask, int64_t n,
                        hipStream_t stream);
// Stable sort of u64 keys that returns the sorting permutation: the first
// pass generates the payload as the row index, so perm/tmp_perm are only
// buffers.  mask is a superset of the varying key bits, given by the
// caller (no device reduce, no sync).  Nothing is copied back: returns
// true when the result is in (tmp_keys, tmp_perm), false when it is in
// (keys, perm).  1 <= n < 2^31.
bool radix_sort_index32(uint64_t* keys, int32_t* perm, uint64_t* tmp_keys,
                        int32_t* tmp_perm, uint32_t* hist, uint64_t mask,
                        int64_t n, hipStream_t stream);
// histogram buffer size requirement (u32 elements)
int64_t radix_sort_hist_size(int64_t n);
// pass plan the sort runs for a varying-bit mask (OR of key ^ key[0]):
// returns the radix (256, or 512 when HS_RS_9BIT=1 and 9-bit digits save
// a pass) and fills shifts[0..*npass) with the digit shifts, ascending.
int radix_sort_plan(uint64_t mask, int shifts[8], int* npass);

// Fused (bucket, key) sort of the index build, for one integer key column
// (normalize_key dtype codes 0, 1, 4, 5, 6).  The sort key is the
// composite (bucket << shift) | (normalized key - kmin).
// key_minmax: mm[0] = min, mm[1] = max of the normalized keys (device).
void key_minmax(const void* vals, int dtype, int64_t n, uint64_t* mm,
                hipStream_t stream);
// bucket ids must lie in [0, 2^(64 - shift)); shift == 64 needs all zero
void compose_bucket_key(const void* vals, int dtype, const int32_t* buckets,
                        uint64_t kmin, int shift, uint64_t* out, int64_t n,
                        hipStream_t stream);
// the key column of the sorted rows, from the sorted composite:
// ((c & low_mask) + kmin) un-normalized, cast to the column's dtype
void restore_key(const uint64_t* sorted, uint64_t low_mask, uint64_t kmin,
                 int dtype, void* out, int64_t n, hipStream_t stream);
// seg[b] = lower bound of (b << shift) in the sorted composite for
// b < num_buckets, seg[num_buckets] = n (num_buckets + 1 entries)
void bucket_seg_offsets(const uint64_t* sorted, int64_t n, int shift,
                        int32_t num_buckets, int64_t* seg,
                        hipStream_t stream);

// K4: segmented sorted merge join, two-phase per-tile form.  Phase 1
// writes one pair-count per 256-row left tile; after an exclusive scan
// of tile counts, phase 2 recomputes the tile-narrowed searches and
// emits pairs at tile_offset + intra-tile LDS prefix (no per-row
// metadata arrays touch HBM).
int64_t merge_join_tile_size();
// K4b: segmented two-sorted-run merge permutation (split[b] = A/B
// boundary per bucket; == seg[b+1] for single-run buckets).
void run_merge_perm(const uint64_t* keys, const int64_t* seg,
                    const int64_t* split, int64_t n, int64_t n_seg,
                    int64_t* perm, hipStream_t stream);
void merge_join_tile_count(const uint64_t* lkeys, const uint64_t* rkeys,
                           const int64_t* lseg, const int64_t* rseg,
                           int64_t n_left, int64_t n_seg,
                           int64_t* tile_counts, hipStream_t stream);
void merge_join_tile_emit(const uint64_t* lkeys, const uint64_t* rkeys,
                          const int64_t* lseg, const int64_t* rseg,
                          int64_t n_left, int64_t n_seg,
                          const int64_t* tile_offsets, int64_t* out_l,
                          int64_t* out_r, hipStream_t stream);
// Join modes of the tile join (compile-time instantiations of the same
// two kernels).  With c = a left row's match count, the row takes
// e slots: INNER c; LEFT_OUTER max(c, 1), the single pair (i, -1) when
// c == 0; LEFT_SEMI c > 0; LEFT_ANTI c == 0.  tile_counts hold sums of
// e.  Semi and anti write only out_l (out_r may be null).  The overloads
// without ``mode`` above are the INNER join.
enum MergeJoinMode : int {
  MERGE_JOIN_INNER = 0,
  MERGE_JOIN_LEFT_OUTER = 1,
  MERGE_JOIN_LEFT_SEMI = 2,
  MERGE_JOIN_LEFT_ANTI = 3,
};
void merge_join_tile_count(const uint64_t* lkeys, const uint64_t* rkeys,
                           const int64_t* lseg, const int64_t* rseg,
                           int64_t n_left, int64_t n_seg, int mode,
                           int64_t* tile_counts, hipStream_t stream);
void merge_join_tile_emit(const uint64_t* lkeys, const uint64_t* rkeys,
                          const int64_t* lseg, const int64_t* rseg,
                          int64_t n_left, int64_t n_seg, int mode,
                          const int64_t* tile_offsets, int64_t* out_l,
                          int64_t* out_r, hipStream_t stream);

// generic exclusive scan over i64 (single pass, device-wide)
void exclusive_scan_i64(const int64_t* in, int64_t* out, int64_t n,
                        int64_t* total, hipStream_t stream);

// filter scan: indices i (ascending) with lo <= key[i] <= hi (u64 order,
// inclusive flags).  Two-phase: count (fills block_counts, scans them in
// place, writes total) then emit (stable compaction using the scanned
// block bases).  block_counts sized select_num_blocks(n).
int64_t select_num_blocks(int64_t n);
void select_range_count(const uint64_t* keys, int64_t n, uint64_t lo,
                        uint64_t hi, bool lo_incl, bool hi_incl,
                        int64_t* block_counts, int64_t* total,
                        hipStream_t stream);
void select_range_emit(const uint64_t* keys, int64_t n, uint64_t lo,
                       uint64_t hi, bool lo_incl, bool hi_incl,
                       const int64_t* block_bases, int64_t* out_idx,
                       hipStream_t stream);

// K7: membership of values in a sorted set -> bool mask
void isin_sorted(const int64_t* vals, int64_t n, const int64_t* sorted_set,
                 int64_t m, bool* out, hipStream_t stream);

// K8: per-segment min/max of int64 values
void segmented_minmax(const int64_t* vals, const int64_t* seg_off,
                      int64_t n_seg, int64_t* mins, int64_t* maxs,
                      hipStream_t stream);

// K13 (aggregate.hip): group-by over adjacent runs.  Both ops tile the
// ROWS (group_tile_size() rows per tile), never the groups.
int64_t group_tile_size();
// group offsets, two-phase like select_range: count writes the number of
// group heads per tile; after an exclusive scan of the tile counts
// (exclusive_scan_i64, total = n_groups) emit writes the head row of every
// group in ascending order and out[n_groups] = n.  keys: 1..8 host arrays
// of device pointers to normalized u64 columns; masks: nullptr, or per
// column validity bytes / nullptr.  Row i heads a group if i == 0 or any
// column's (null flag, key) differs from row i - 1; the stored key of a
// null row is ignored.  Key and mask pointers must be 16-byte aligned.
void group_offsets_count(const uint64_t* const* keys,
                         const uint8_t* const* masks, int n_cols, int64_t n,
                         int64_t* tile_counts, hipStream_t stream);
void group_offsets_emit(const uint64_t* const* keys,
                        const uint8_t* const* masks, int n_cols, int64_t n,
                        const int64_t* tile_offsets, const int64_t* total,
                        int64_t* out, hipStream_t stream);
// fused segmented reduce: per group [offsets[g], offsets[g+1]) the sum,
// min, max and valid-count of vals in one read.  dtype: 0=i64, 1=i32,
// 2=f64, 3=f32.  sums are i64 (wrapping) for integers and f64 for floats;
// mins/maxs have the input type and follow normalize_key order; any of
// sums/mins/maxs may be null, counts is required.  A group with no valid
// row gets count 0 and zeros.  valid: validity bytes or nullptr.  offsets
// must ascend strictly from 0 to n.  tile_groups: n_tiles + 1 scratch
// entries; partials: 4 * segmented_reduce_num_blocks(n) scratch entries.
// vals and valid must be 16-byte aligned.  No atomics: float sums are
// bitwise reproducible.
int64_t segmented_reduce_num_blocks(int64_t n);
void segmented_reduce(const void* vals, int dtype, const uint8_t* valid,
                      const int64_t* offsets, int64_t n, int64_t n_groups,
                      void* sums, void* mins, void* maxs, int64_t* counts,
                      int64_t* tile_groups, int64_t* partials,
                      hipStream_t stream);

// K14 (topk.hip): rows of the k smallest keys, without sorting.  Over the
// rows with valid[i] != 0 (all rows when valid is null) let T be the k-th
// smallest key in u64 order.  The result is, in ascending row index, every
// valid row with key < T and then of the rows with key == T either all of
// them (keep_ties) or the first k - #less in row order.  k > n_valid gives
// every valid row.  The stored key of an invalid row is ignored.
// Two-phase like select_range: topk_select finds T (MSD radix select,
// 8-bit digits, no host read between passes) and counts; it returns the
// device address of the output length.  After reading it the caller sizes
// out and runs topk_emit with the same keys, valid and scratch.
// n >= 1, 1 <= k <= n.  scratch: topk_scratch_size(n) int64 entries, ZEROED
// by the caller.  keys and valid must be 16-byte aligned.
int64_t topk_tile_size();
int64_t topk_num_blocks(int64_t n);
int64_t topk_scratch_size(int64_t n);
int64_t* topk_select(const uint64_t* keys, const uint8_t* valid, int64_t n,
                     int64_t k, bool keep_ties, int64_t* scratch,
                     hipStream_t stream);
void topk_emit(const uint64_t* keys, const uint8_t* valid, int64_t n,
               const int64_t* scratch, int64_t* out, int64_t n_out,
               hipStream_t stream);

// K8: bloom filter build/probe (k hashes, m_bits bits over u64 words)
void bloom_build(const int64_t* vals, int64_t n, uint64_t* words,
                 int64_t m_bits, int k, hipStream_t stream);
void bloom_probe(const int64_t* vals, int64_t n, const uint64_t* words,
                 int64_t m_bits, int k, bool* out, hipStream_t stream);
// K9: batched device sketch-predicate probe — every value against every
// per-file filter; out[f] |= filter f may contain any value
void bloom_probe_many(const int64_t* vals, int64_t n_vals,
                      const uint64_t* words, int64_t words_per_filter,
                      int64_t n_filters, int64_t m_bits, int k, bool* out,
                      hipStream_t stream);

// K10: z-order bit interleave of up to 8 normalized u64 columns
void zorder_key(const uint64_t* const* cols, int n_cols, int bits_per_col,
                int64_t n, uint64_t* out, hipStream_t stream);

// row gather: out[i] = in[idx[i]] for element sizes 1/2/4/8, through an
// int64 or an int32 index
void gather(const void* in, const int64_t* idx, void* out, int64_t n,
            int elem_size, hipStream_t stream);
void gather(const void* in, const int32_t* idx, void* out, int64_t n,
            int elem_size, hipStream_t stream);

// K1 parquet dictionary-page decode: expand an RLE/bit-packed hybrid
// run table (host-parsed) into u32 dictionary indices.
// runs arrays (one entry per run):
//   kind: 0 = repeated (value in run_value), 1 = bit-packed literal
//         (bits start at src bit offset run_payload_bitoff)
//   out_off: first output index of the run; len: output count
void rle_decode_indices(const uint8_t* src, const int64_t* run_kind,
                        const int64_t* run_out_off,
                        const int64_t* run_len,
                        const int64_t* run_payload_bitoff,
                        const int64_t* run_value, int64_t n_runs,
                        int bit_width, uint32_t* out, int64_t n_out,
                        hipStream_t stream);

// K1 parquet page decode: copy nbytes from (src + src_off) — any byte
// alignment — to 4-byte-aligned dst+dst_off.  nbytes % 4 == 0.  The src
// buffer must extend >= 4 bytes past src_off+nbytes (parquet footers
// guarantee this for page payloads).
// K1 snappy raw-block page decompression: one wave per page; status[p]
// = 0 on success, nonzero on malformed input (caller falls back).
void snappy_decompress_pages(const uint8_t* src, const int64_t* src_off,
                             const int64_t* src_end, uint8_t* dst,
                             const int64_t* dst_off,
                             const int64_t* dst_len, int32_t* status,
                             int n_pages, hipStream_t stream);

void copy_unaligned(const uint8_t* src, int64_t src_off, uint8_t* dst,
                    int64_t dst_off, int64_t nbytes, hipStream_t stream);

}  // namespace hsk
