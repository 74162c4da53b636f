// Torch extension binding for the CDNA4 kernel suite (kernels.hip).
// Written directly against the ROCm torch C++ surface (c10::hip) — no
// CUDA-compat naming, no hipify.

#include <torch/extension.h>

#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <string>
#include <tuple>
#include <vector>

#include "bucket_writer.h"
#include "kernels/kernels.h"

namespace {

hipStream_t current_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

void check_cuda(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

int normalize_dtype_code(torch::ScalarType t) {
  switch (t) {
    case torch::kInt64: return 0;
    case torch::kInt32: return 1;
    case torch::kFloat64: return 2;
    case torch::kFloat32: return 3;
    case torch::kInt16: return 4;
    case torch::kInt8: return 5;
    case torch::kBool: return 6;
    default:
      TORCH_CHECK(false, "unsupported sort-key dtype");
  }
}

torch::Tensor murmur3_bucket(std::vector<torch::Tensor> keys,
                             int64_t num_buckets,
                             std::vector<torch::Tensor> masks = {}) {
  TORCH_CHECK(!keys.empty(), "need at least one key column");
  TORCH_CHECK(masks.empty() || masks.size() == keys.size(),
              "masks must be empty or parallel to keys");
  // pmod by zero is undefined in the kernel
  TORCH_CHECK(num_buckets > 0 && num_buckets <= (int64_t)INT32_MAX,
              "murmur3_bucket: num_buckets must be in 1..INT32_MAX, got ",
              num_buckets);
  auto n = keys[0].numel();
  auto dev = keys[0].device();
  // the running hash reaches HBM only between columns: the last column's
  // kernel applies the pmod to the hash in its register
  torch::Tensor h;
  if (keys.size() > 1)
    h = torch::empty({n}, torch::dtype(torch::kInt32).device(dev));
  auto out = torch::empty({n}, torch::dtype(torch::kInt32).device(dev));
  auto stream = current_stream();
  bool first = true;
  for (size_t ci = 0; ci < keys.size(); ++ci) {
    auto& k = keys[ci];
    check_cuda(k, "key");
    TORCH_CHECK(k.numel() == n, "key column length mismatch");
    torch::Tensor col = k;
    int kind;
    switch (col.scalar_type()) {
      case torch::kInt64:
        kind = 1;
        break;
      case torch::kFloat64:
        kind = 3;  // hashed as canonical bits: -0.0 as 0.0, one NaN
        break;
      case torch::kInt32:
        kind = 0;
        break;
      case torch::kFloat32:
        kind = 2;
        break;
      case torch::kInt16:
      case torch::kInt8:
      case torch::kBool:
        col = col.to(torch::kInt32);
        kind = 0;
        break;
      default:
        TORCH_CHECK(false, "unsupported hash-key dtype");
    }
    // an empty mask tensor means "column has no nulls"
    const uint8_t* valid = nullptr;
    torch::Tensor mcol;
    if (!masks.empty() && masks[ci].numel() > 0) {
      mcol = masks[ci];
      check_cuda(mcol, "mask");
      TORCH_CHECK(mcol.numel() == n, "mask length mismatch");
      TORCH_CHECK(mcol.scalar_type() == torch::kBool ||
                      mcol.scalar_type() == torch::kUInt8,
                  "mask must be bool/uint8");
      valid = (const uint8_t*)mcol.data_ptr();
    }
    uint32_t* hp =
        h.defined() ? (uint32_t*)h.data_ptr<int32_t>() : nullptr;
    if (ci + 1 < keys.size())
      hsk::murmur3_column(col.data_ptr(), kind, valid, hp, n, first,
                          /*seed=*/42u, stream);
    else
      hsk::murmur3_last_column(col.data_ptr(), kind, valid, hp,
                               out.data_ptr<int32_t>(), n, first,
                               /*seed=*/42u, (int32_t)num_buckets, stream);
    first = false;
  }
  return out;
}

torch::Tensor normalize_key(torch::Tensor vals, bool canonical = false,
                            bool descending = false) {
  check_cuda(vals, "vals");
  auto n = vals.numel();
  auto out = torch::empty(
      {n}, torch::dtype(torch::kInt64).device(vals.device()));
  hsk::normalize_key(vals.data_ptr(),
                     normalize_dtype_code(vals.scalar_type()),
                     (uint64_t*)out.data_ptr<int64_t>(), n,
                     current_stream(), canonical, descending);
  return out;
}

std::tuple<torch::Tensor, torch::Tensor> radix_sort_pairs(
    torch::Tensor keys, torch::Tensor payload) {
  check_cuda(keys, "keys");
  check_cuda(payload, "payload");
  TORCH_CHECK(keys.scalar_type() == torch::kInt64, "keys must be int64");
  TORCH_CHECK(payload.scalar_type() == torch::kInt64,
              "payload must be int64");
  auto n = keys.numel();
  auto out_keys = keys.clone();
  if (n <= 1) return {out_keys, payload.clone()};
  auto hist = torch::empty({hsk::radix_sort_hist_size(n)},
                           torch::dtype(torch::kInt32).device(keys.device()));
  auto mask = torch::empty({1},
                           torch::dtype(torch::kInt64).device(keys.device()));
  auto tmp_keys = torch::empty_like(keys);
  // payload values are row indices in every engine call site: when they
  // fit int32 the sort runs the narrow-payload pipeline (2/3 the
  // per-pass traffic) and widens at the end
  bool fits32 = n < (int64_t)INT32_MAX;
  if (fits32) {
    auto mm = payload.aminmax();
    fits32 = std::get<0>(mm).item<int64_t>() >= 0 &&
             std::get<1>(mm).item<int64_t>() < (int64_t)INT32_MAX;
  }
  if (fits32) {
    auto p32 = payload.to(torch::kInt32);
    auto tmp_p32 = torch::empty_like(p32);
    hsk::radix_sort_pairs32((uint64_t*)out_keys.data_ptr<int64_t>(),
                            p32.data_ptr<int32_t>(),
                            (uint64_t*)tmp_keys.data_ptr<int64_t>(),
                            tmp_p32.data_ptr<int32_t>(),
                            (uint32_t*)hist.data_ptr<int32_t>(),
                            (uint64_t*)mask.data_ptr<int64_t>(), n,
                            current_stream());
    return {out_keys, p32.to(torch::kInt64)};
  }
  auto out_payload = payload.clone();
  auto tmp_payload = torch::empty_like(payload);
  hsk::radix_sort_pairs((uint64_t*)out_keys.data_ptr<int64_t>(),
                        out_payload.data_ptr<int64_t>(),
                        (uint64_t*)tmp_keys.data_ptr<int64_t>(),
                        tmp_payload.data_ptr<int64_t>(),
                        (uint32_t*)hist.data_ptr<int32_t>(),
                        (uint64_t*)mask.data_ptr<int64_t>(), n,
                        current_stream());
  return {out_keys, out_payload};
}

// The pass plan the sort runs for a varying-bit mask: (radix, shifts).
// Thin wrapper over the planner both payload widths call, so a test can
// see which digit width a process runs (HS_RS_9BIT is read once).
std::tuple<int64_t, std::vector<int64_t>> radix_sort_plan(uint64_t mask) {
  int shifts[8];
  int npass = 0;
  int radix = hsk::radix_sort_plan(mask, shifts, &npass);
  return {(int64_t)radix, std::vector<int64_t>(shifts, shifts + npass)};
}

// Device-wide exclusive scan of an int64 tensor: (out, total), total a
// 1-element device tensor.
std::tuple<torch::Tensor, torch::Tensor> exclusive_scan(torch::Tensor t) {
  check_cuda(t, "t");
  TORCH_CHECK(t.scalar_type() == torch::kInt64, "t must be int64");
  auto out = torch::empty_like(t);
  auto total = torch::empty(
      {1}, torch::dtype(torch::kInt64).device(t.device()));
  hsk::exclusive_scan_i64(t.data_ptr<int64_t>(), out.data_ptr<int64_t>(),
                          t.numel(), total.data_ptr<int64_t>(),
                          current_stream());
  return {out, total};
}

// mode: hsk::MergeJoinMode (0 inner, 1 left outer, 2 left semi, 3 left
// anti).  Semi and anti return an empty second tensor.
std::tuple<torch::Tensor, torch::Tensor> merge_join(torch::Tensor lkeys,
                                                    torch::Tensor rkeys,
                                                    torch::Tensor lseg,
                                                    torch::Tensor rseg,
                                                    int64_t mode) {
  check_cuda(lkeys, "lkeys");
  check_cuda(rkeys, "rkeys");
  TORCH_CHECK(mode >= hsk::MERGE_JOIN_INNER &&
                  mode <= hsk::MERGE_JOIN_LEFT_ANTI,
              "merge_join: unknown mode ", mode);
  bool pairs = mode == hsk::MERGE_JOIN_INNER ||
               mode == hsk::MERGE_JOIN_LEFT_OUTER;
  auto dev = lkeys.device();
  auto opts = torch::dtype(torch::kInt64).device(dev);
  // segment offsets may arrive on CPU
  auto lseg_d = lseg.to(dev, torch::kInt64).contiguous();
  auto rseg_d = rseg.to(dev, torch::kInt64).contiguous();
  int64_t n_left = lkeys.numel();
  int64_t n_seg = lseg_d.numel() - 1;
  auto stream = current_stream();
  if (n_left == 0) {
    return {torch::empty({0}, opts), torch::empty({0}, opts)};
  }
  if (rkeys.numel() == 0) {
    // nothing can match: inner and semi are empty, outer and anti keep
    // every left row (null-extended for outer) without a launch
    if (mode == hsk::MERGE_JOIN_INNER || mode == hsk::MERGE_JOIN_LEFT_SEMI)
      return {torch::empty({0}, opts), torch::empty({0}, opts)};
    return {torch::arange(n_left, opts),
            pairs ? torch::full({n_left}, -1, opts)
                  : torch::empty({0}, opts)};
  }
  int64_t tile = hsk::merge_join_tile_size();
  int64_t n_tiles = (n_left + tile - 1) / tile;
  auto tile_counts = torch::empty({n_tiles}, opts);
  hsk::merge_join_tile_count((const uint64_t*)lkeys.data_ptr<int64_t>(),
                             (const uint64_t*)rkeys.data_ptr<int64_t>(),
                             lseg_d.data_ptr<int64_t>(),
                             rseg_d.data_ptr<int64_t>(), n_left, n_seg,
                             (int)mode, tile_counts.data_ptr<int64_t>(),
                             stream);
  auto tile_offsets = torch::empty({n_tiles}, opts);
  auto total = torch::empty({1}, opts);
  hsk::exclusive_scan_i64(tile_counts.data_ptr<int64_t>(),
                          tile_offsets.data_ptr<int64_t>(), n_tiles,
                          total.data_ptr<int64_t>(), stream);
  int64_t n_out = total.cpu().item<int64_t>();
  auto out_l = torch::empty({n_out}, opts);
  auto out_r = torch::empty({pairs ? n_out : 0}, opts);
  if (n_out > 0) {
    hsk::merge_join_tile_emit((const uint64_t*)lkeys.data_ptr<int64_t>(),
                              (const uint64_t*)rkeys.data_ptr<int64_t>(),
                              lseg_d.data_ptr<int64_t>(),
                              rseg_d.data_ptr<int64_t>(), n_left, n_seg,
                              (int)mode, tile_offsets.data_ptr<int64_t>(),
                              out_l.data_ptr<int64_t>(),
                              pairs ? out_r.data_ptr<int64_t>() : nullptr,
                              stream);
  }
  return {out_l, out_r};
}

torch::Tensor isin_sorted(torch::Tensor vals, torch::Tensor sorted_set) {
  check_cuda(vals, "vals");
  auto n = vals.numel();
  auto out = torch::empty(
      {n}, torch::dtype(torch::kBool).device(vals.device()));
  if (sorted_set.numel() == 0) {
    out.zero_();
    return out;
  }
  auto set_d = sorted_set.to(vals.device(), torch::kInt64).contiguous();
  hsk::isin_sorted(vals.data_ptr<int64_t>(), n, set_d.data_ptr<int64_t>(),
                   set_d.numel(), out.data_ptr<bool>(), current_stream());
  return out;
}

std::tuple<torch::Tensor, torch::Tensor> segmented_minmax(
    torch::Tensor vals, torch::Tensor seg_off) {
  check_cuda(vals, "vals");
  auto seg_d = seg_off.to(vals.device(), torch::kInt64).contiguous();
  int64_t n_seg = seg_d.numel() - 1;
  auto opts = torch::dtype(torch::kInt64).device(vals.device());
  auto mins = torch::empty({n_seg}, opts);
  auto maxs = torch::empty({n_seg}, opts);
  hsk::segmented_minmax(vals.data_ptr<int64_t>(), seg_d.data_ptr<int64_t>(),
                        n_seg, mins.data_ptr<int64_t>(),
                        maxs.data_ptr<int64_t>(), current_stream());
  return {mins, maxs};
}

// the kernels take pos % m_bits: m_bits == 0 is undefined
void check_bloom_args(int64_t m_bits, int64_t k) {
  TORCH_CHECK(m_bits > 0 && k >= 0 && k <= (int64_t)INT32_MAX,
              "bloom: need m_bits > 0 and k >= 0, got m_bits=", m_bits,
              " k=", k);
}

torch::Tensor bloom_build(torch::Tensor vals, int64_t m_bits, int64_t k) {
  check_cuda(vals, "vals");
  check_bloom_args(m_bits, k);
  int64_t words = (m_bits + 63) / 64;
  auto out = torch::zeros(
      {words}, torch::dtype(torch::kInt64).device(vals.device()));
  hsk::bloom_build(vals.data_ptr<int64_t>(), vals.numel(),
                   (uint64_t*)out.data_ptr<int64_t>(), m_bits, (int)k,
                   current_stream());
  return out;
}

torch::Tensor bloom_probe(torch::Tensor vals, torch::Tensor words,
                          int64_t m_bits, int64_t k) {
  check_cuda(vals, "vals");
  check_bloom_args(m_bits, k);
  auto words_d = words.to(vals.device(), torch::kInt64).contiguous();
  auto out = torch::empty(
      {vals.numel()}, torch::dtype(torch::kBool).device(vals.device()));
  hsk::bloom_probe(vals.data_ptr<int64_t>(), vals.numel(),
                   (const uint64_t*)words_d.data_ptr<int64_t>(), m_bits,
                   (int)k, out.data_ptr<bool>(), current_stream());
  return out;
}

torch::Tensor bloom_probe_many(torch::Tensor vals, torch::Tensor words,
                               int64_t m_bits, int64_t k) {
  check_cuda(vals, "vals");
  check_bloom_args(m_bits, k);
  TORCH_CHECK(words.dim() == 2, "words must be [n_filters, words]");
  auto words_d = words.to(vals.device(), torch::kInt64).contiguous();
  int64_t n_filters = words_d.size(0);
  auto out = torch::zeros(
      {n_filters}, torch::dtype(torch::kBool).device(vals.device()));
  hsk::bloom_probe_many(vals.data_ptr<int64_t>(), vals.numel(),
                        (const uint64_t*)words_d.data_ptr<int64_t>(),
                        words_d.size(1), n_filters, m_bits, (int)k,
                        out.data_ptr<bool>(), current_stream());
  return out;
}

torch::Tensor zorder_key(std::vector<torch::Tensor> cols,
                         int64_t bits_per_col) {
  TORCH_CHECK(!cols.empty() && cols.size() <= 8, "1..8 zorder columns");
  // the kernel shifts by 63 - (b * n_cols + c): past 64 bits is undefined
  TORCH_CHECK(bits_per_col >= 0 &&
                  (int64_t)cols.size() * bits_per_col <= 64,
              "zorder_key: need bits_per_col >= 0 and n_cols * "
              "bits_per_col <= 64, got ", cols.size(), " x ", bits_per_col);
  auto n = cols[0].numel();
  std::vector<const uint64_t*> ptrs;
  for (auto& c : cols) {
    check_cuda(c, "zorder col");
    ptrs.push_back((const uint64_t*)c.data_ptr<int64_t>());
  }
  auto out = torch::empty(
      {n}, torch::dtype(torch::kInt64).device(cols[0].device()));
  hsk::zorder_key(ptrs.data(), (int)ptrs.size(), (int)bits_per_col, n,
                  (uint64_t*)out.data_ptr<int64_t>(), current_stream());
  return out;
}

torch::Tensor run_merge_perm(torch::Tensor keys, torch::Tensor seg,
                             torch::Tensor split) {
  check_cuda(keys, "keys");
  TORCH_CHECK(keys.scalar_type() == torch::kInt64, "keys must be int64");
  auto dev = keys.device();
  auto i64 = torch::dtype(torch::kInt64);
  auto seg_d = seg.to(dev, torch::kInt64).contiguous();
  auto split_d = split.to(dev, torch::kInt64).contiguous();
  int64_t n = keys.numel();
  int64_t n_seg = seg_d.numel() - 1;
  TORCH_CHECK(split_d.numel() == n_seg, "split must have n_seg entries");
  auto perm = torch::empty({n}, i64.device(dev));
  hsk::run_merge_perm((const uint64_t*)keys.data_ptr<int64_t>(),
                      seg_d.data_ptr<int64_t>(),
                      split_d.data_ptr<int64_t>(), n, n_seg,
                      perm.data_ptr<int64_t>(), current_stream());
  return perm;
}

torch::Tensor snappy_decompress(torch::Tensor dev_bytes,
                                torch::Tensor src_off,
                                torch::Tensor src_end, torch::Tensor dst,
                                torch::Tensor dst_off,
                                torch::Tensor dst_len) {
  check_cuda(dev_bytes, "dev_bytes");
  check_cuda(dst, "dst");
  TORCH_CHECK(dev_bytes.scalar_type() == torch::kUInt8 &&
                  dst.scalar_type() == torch::kUInt8,
              "byte tensors required");
  int64_t n_pages = src_off.numel();
  auto dev = dev_bytes.device();
  auto i64 = torch::dtype(torch::kInt64).device(dev);
  auto so = src_off.to(i64.device(), torch::kInt64).contiguous();
  auto se = src_end.to(i64.device(), torch::kInt64).contiguous();
  auto dofs = dst_off.to(i64.device(), torch::kInt64).contiguous();
  auto dl = dst_len.to(i64.device(), torch::kInt64).contiguous();
  auto status = torch::zeros(
      {n_pages}, torch::dtype(torch::kInt32).device(dev));
  hsk::snappy_decompress_pages(
      dev_bytes.data_ptr<uint8_t>(), so.data_ptr<int64_t>(),
      se.data_ptr<int64_t>(), dst.data_ptr<uint8_t>(),
      dofs.data_ptr<int64_t>(), dl.data_ptr<int64_t>(),
      status.data_ptr<int32_t>(), (int)n_pages, current_stream());
  return status;
}

// Host decode of RLE-hybrid definition levels (max_def = 1) into a
// validity byte array: the per-page Python decoder costs ~1 ms/page on
// pyarrow's many-run encodings; this tight loop is ~20 us.
torch::Tensor decode_def_levels(py::buffer data, int64_t off,
                                int64_t length, int64_t n) {
  py::buffer_info info = data.request();
  const uint8_t* base = (const uint8_t*)info.ptr;
  TORCH_CHECK(off >= 0 && off + length <= (int64_t)info.size,
              "def-levels out of range");
  const uint8_t* p = base + off;
  const uint8_t* end = p + length;
  auto out = torch::empty({n}, torch::dtype(torch::kBool));
  bool* o = out.data_ptr<bool>();
  int64_t filled = 0;
  while (filled < n && p < end) {
    uint64_t header = 0;
    int shift = 0;
    while (true) {
      TORCH_CHECK(p < end, "def-levels: truncated varint");
      uint8_t b = *p++;
      header |= (uint64_t)(b & 0x7F) << shift;
      if (!(b & 0x80)) break;
      shift += 7;
    }
    if (header & 1) {  // bit-packed run: groups of 8 levels
      int64_t groups = (int64_t)(header >> 1);
      int64_t cnt = groups * 8;
      if (cnt > n - filled) cnt = n - filled;
      TORCH_CHECK(p + groups <= end, "def-levels: truncated bitpack");
      for (int64_t i = 0; i < cnt; ++i)
        o[filled + i] = (p[i >> 3] >> (i & 7)) & 1;
      p += groups;
      filled += cnt;
    } else {  // RLE run: one value byte at bit width 1
      int64_t run = (int64_t)(header >> 1);
      if (run > n - filled) run = n - filled;
      TORCH_CHECK(p < end, "def-levels: truncated rle value");
      bool v = *p++ != 0;
      std::fill(o + filled, o + filled + run, v);
      filled += run;
    }
  }
  std::fill(o + filled, o + n, true);
  return out;
}

// Batched RLE-hybrid run parse over MANY pages in one GIL-released
// call: the per-page python loop cost dominated multi-row-group snappy
// chunk decode (hundreds of pages x ~0.5 ms of interpreter work).
// Emits runs already shifted into the caller's output-row and
// bit-offset coordinate spaces, plus per-page run counts.
std::vector<torch::Tensor> parse_rle_runs_batch(
    torch::Tensor bytes, torch::Tensor starts, torch::Tensor ends,
    torch::Tensor bws, torch::Tensor n_valids, torch::Tensor out_shifts,
    torch::Tensor bit_shifts) {
  TORCH_CHECK(!bytes.is_cuda() && bytes.scalar_type() == torch::kUInt8,
              "bytes must be a cpu u8 tensor");
  const uint8_t* d = bytes.data_ptr<uint8_t>();
  int64_t n_pages = starts.numel();
  auto sa = starts.data_ptr<int64_t>();
  auto ea = ends.data_ptr<int64_t>();
  auto ba = bws.data_ptr<int64_t>();
  auto va = n_valids.data_ptr<int64_t>();
  auto oa = out_shifts.data_ptr<int64_t>();
  auto fa = bit_shifts.data_ptr<int64_t>();
  std::vector<int64_t> kind, out_off, len, bitoff, value, counts;
  counts.reserve(n_pages);
  for (int64_t pg = 0; pg < n_pages; ++pg) {
    int64_t pos = sa[pg], end = ea[pg], out = 0;
    int64_t bit_width = ba[pg], num_values = va[pg];
    int64_t bw_bytes = (bit_width + 7) / 8;
    int64_t n_runs0 = (int64_t)kind.size();
    while (out < num_values && pos < end) {
      uint64_t h = 0;
      int shift = 0;
      while (true) {
        TORCH_CHECK(pos < end, "rle: truncated varint");
        uint8_t b = d[pos++];
        h |= (uint64_t)(b & 0x7F) << shift;
        if (!(b & 0x80)) break;
        shift += 7;
      }
      if (h & 1) {
        int64_t groups = (int64_t)(h >> 1);
        int64_t count = groups * 8;
        if (count > num_values - out) count = num_values - out;
        kind.push_back(1);
        out_off.push_back(out + oa[pg]);
        len.push_back(count);
        bitoff.push_back(pos * 8 + fa[pg]);
        value.push_back(0);
        pos += groups * bit_width;
        out += count;
      } else {
        int64_t run = (int64_t)(h >> 1);
        if (run > num_values - out) run = num_values - out;
        int64_t v = 0;
        for (int64_t i = 0; i < bw_bytes; i++) {
          TORCH_CHECK(pos < end, "rle: truncated repeat value");
          v |= (int64_t)d[pos++] << (8 * i);
        }
        kind.push_back(0);
        out_off.push_back(out + oa[pg]);
        len.push_back(run);
        bitoff.push_back(0);
        value.push_back(v);
        out += run;
      }
    }
    TORCH_CHECK(out == num_values, "rle: page ", pg, " produced ", out,
                " of ", num_values, " values");
    counts.push_back((int64_t)kind.size() - n_runs0);
  }
  auto opts = torch::dtype(torch::kInt64);
  auto mk = [&](std::vector<int64_t>& v) { return torch::tensor(v, opts); };
  return {mk(kind), mk(out_off), mk(len), mk(bitoff), mk(value),
          mk(counts)};
}

// PLAIN BYTE_ARRAY page parse (K1 string path): each value is a 4-byte
// little-endian length prefix + payload.  Concatenates the values of
// every listed page into one arrow-style (int32 offsets, bytes) pair so
// the caller can dictionary-encode in one pass (parquet-format.md
// Encodings: PLAIN for BYTE_ARRAY; reference uses parquet-mr's reader).
std::vector<torch::Tensor> parse_byte_arrays(
    torch::Tensor bytes, torch::Tensor starts, torch::Tensor ends,
    torch::Tensor counts) {
  TORCH_CHECK(!bytes.is_cuda() && bytes.scalar_type() == torch::kUInt8,
              "bytes must be a cpu u8 tensor");
  const uint8_t* d = bytes.data_ptr<uint8_t>();
  int64_t n_pages = starts.numel();
  auto sa = starts.data_ptr<int64_t>();
  auto ea = ends.data_ptr<int64_t>();
  auto ca = counts.data_ptr<int64_t>();
  int64_t total_n = 0, cap = 0;
  for (int64_t p = 0; p < n_pages; ++p) {
    total_n += ca[p];
    cap += ea[p] - sa[p];
  }
  TORCH_CHECK(cap <= INT32_MAX, "byte-array payload exceeds int32 offsets");
  auto offs = torch::empty({total_n + 1}, torch::dtype(torch::kInt32));
  auto out = torch::empty({cap}, torch::dtype(torch::kUInt8));
  int32_t* op = offs.data_ptr<int32_t>();
  uint8_t* bp = out.data_ptr<uint8_t>();
  int64_t written = 0, vi = 0;
  for (int64_t p = 0; p < n_pages; ++p) {
    int64_t pos = sa[p], end = ea[p];
    for (int64_t k = 0; k < ca[p]; ++k) {
      TORCH_CHECK(pos + 4 <= end, "byte-array page ", p,
                  ": truncated length prefix");
      uint32_t len = (uint32_t)d[pos] | ((uint32_t)d[pos + 1] << 8) |
                     ((uint32_t)d[pos + 2] << 16) |
                     ((uint32_t)d[pos + 3] << 24);
      pos += 4;
      TORCH_CHECK(pos + (int64_t)len <= end, "byte-array page ", p,
                  ": value overruns page");
      op[vi++] = (int32_t)written;
      memcpy(bp + written, d + pos, len);
      written += len;
      pos += len;
    }
  }
  op[vi] = (int32_t)written;
  return {offs, out.narrow(0, 0, written)};
}

// GIL-released memcpy of a buffer-protocol object (e.g. a pyarrow
// Buffer from Codec::Decompress) into a cpu uint8 tensor slice — a
// plain numpy slice assignment holds the GIL for the whole copy, which
// serializes the 16-thread host-codec upload staging.
void host_memcpy(torch::Tensor dst, int64_t off, py::buffer src) {
  TORCH_CHECK(!dst.is_cuda() && dst.scalar_type() == torch::kUInt8,
              "dst must be a cpu u8 tensor");
  py::buffer_info info = src.request();
  int64_t n = (int64_t)info.size * (int64_t)info.itemsize;
  TORCH_CHECK(off >= 0 && off + n <= dst.numel(),
              "host_memcpy out of range");
  uint8_t* d = dst.data_ptr<uint8_t>() + off;
  const void* s = info.ptr;
  {
    py::gil_scoped_release rel;
    memcpy(d, s, (size_t)n);
  }
}

std::vector<torch::Tensor> parse_rle_runs(torch::Tensor bytes,
                                           int64_t start, int64_t end,
                                           int64_t bit_width,
                                           int64_t num_values) {
  TORCH_CHECK(!bytes.is_cuda() && bytes.scalar_type() == torch::kUInt8,
              "bytes must be a cpu u8 tensor");
  const uint8_t* d = bytes.data_ptr<uint8_t>();
  std::vector<int64_t> kind, out_off, len, bitoff, value;
  int64_t pos = start, out = 0;
  int64_t bw_bytes = (bit_width + 7) / 8;
  while (out < num_values && pos < end) {
    // varint header
    uint64_t h = 0;
    int shift = 0;
    while (true) {
      TORCH_CHECK(pos < end, "rle: truncated varint");
      uint8_t b = d[pos++];
      h |= (uint64_t)(b & 0x7F) << shift;
      if (!(b & 0x80)) break;
      shift += 7;
    }
    if (h & 1) {
      int64_t groups = (int64_t)(h >> 1);
      int64_t count = groups * 8;
      if (count > num_values - out) count = num_values - out;
      kind.push_back(1);
      out_off.push_back(out);
      len.push_back(count);
      bitoff.push_back(pos * 8);
      value.push_back(0);
      pos += groups * bit_width;  // payload bytes = groups * bit_width
      out += count;
    } else {
      int64_t run = (int64_t)(h >> 1);
      if (run > num_values - out) run = num_values - out;
      int64_t v = 0;
      for (int64_t i = 0; i < bw_bytes; i++) {
        TORCH_CHECK(pos < end, "rle: truncated repeat value");
        v |= (int64_t)d[pos++] << (8 * i);
      }
      kind.push_back(0);
      out_off.push_back(out);
      len.push_back(run);
      bitoff.push_back(0);
      value.push_back(v);
      out += run;
    }
  }
  TORCH_CHECK(out == num_values, "rle: produced ", out, " of ",
              num_values, " values");
  auto opts = torch::dtype(torch::kInt64);
  auto mk = [&](std::vector<int64_t>& v) {
    return torch::tensor(v, opts);
  };
  return {mk(kind), mk(out_off), mk(len), mk(bitoff), mk(value)};
}

torch::Tensor rle_decode(torch::Tensor src_u8_dev, torch::Tensor kind,
                         torch::Tensor out_off, torch::Tensor len,
                         torch::Tensor bitoff, torch::Tensor value,
                         int64_t bit_width, int64_t n_out) {
  check_cuda(src_u8_dev, "src");
  // values are extracted from a 5-byte window into u32 outputs
  TORCH_CHECK(bit_width >= 0 && bit_width <= 32,
              "rle_decode: bit_width must be in 0..32, got ", bit_width);
  auto dev = src_u8_dev.device();
  auto k = kind.to(dev), o = out_off.to(dev), l = len.to(dev),
       b = bitoff.to(dev), v = value.to(dev);
  auto out = torch::empty({n_out},
                          torch::dtype(torch::kInt32).device(dev));
  hsk::rle_decode_indices(src_u8_dev.data_ptr<uint8_t>(),
                          k.data_ptr<int64_t>(), o.data_ptr<int64_t>(),
                          l.data_ptr<int64_t>(), b.data_ptr<int64_t>(),
                          v.data_ptr<int64_t>(), kind.numel(),
                          (int)bit_width,
                          (uint32_t*)out.data_ptr<int32_t>(), n_out,
                          current_stream());
  return out;
}

void copy_unaligned(torch::Tensor src_u8, int64_t src_off,
                    torch::Tensor dst, int64_t dst_byte_off,
                    int64_t nbytes) {
  TORCH_CHECK(src_u8.is_cuda() && dst.is_cuda(), "device tensors required");
  TORCH_CHECK(src_u8.scalar_type() == torch::kUInt8, "src must be u8");
  TORCH_CHECK(src_off + nbytes + 4 <= src_u8.numel(),
              "src buffer must extend 4 bytes past the payload");
  TORCH_CHECK(dst_byte_off % 4 == 0 && nbytes % 4 == 0, "4B granularity");
  hsk::copy_unaligned(src_u8.data_ptr<uint8_t>(), src_off,
                      (uint8_t*)dst.data_ptr(), dst_byte_off, nbytes,
                      current_stream());
}

torch::Tensor gather_rows(torch::Tensor values, torch::Tensor idx) {
  check_cuda(values, "values");
  check_cuda(idx, "idx");
  TORCH_CHECK(idx.scalar_type() == torch::kInt64 ||
                  idx.scalar_type() == torch::kInt32,
              "idx must be int64 or int32");
  auto out = torch::empty({idx.numel()}, values.options());
  if (idx.scalar_type() == torch::kInt32)
    hsk::gather(values.data_ptr(), idx.data_ptr<int32_t>(), out.data_ptr(),
                idx.numel(), (int)values.element_size(), current_stream());
  else
    hsk::gather(values.data_ptr(), idx.data_ptr<int64_t>(), out.data_ptr(),
                idx.numel(), (int)values.element_size(), current_stream());
  return out;
}

int bit_length_u64(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

// Fused (bucket, key) sort for one non-null integer key column: returns
// (perm int32, key column in sorted order, seg int64 on the CPU), or None
// when the key range does not fit beside the bucket bits.  bucket_ids:
// int32 in [0, num_buckets).  The composite (bucket << S) | (key - kmin)
// is sorted once with a generated row-index payload; seg and the sorted
// key column are read back off the sorted composite.
py::object bucket_sort_perm(torch::Tensor key, torch::Tensor bucket_ids,
                            int64_t num_buckets) {
  check_cuda(key, "key");
  check_cuda(bucket_ids, "bucket_ids");
  TORCH_CHECK(bucket_ids.scalar_type() == torch::kInt32,
              "bucket_ids must be int32");
  TORCH_CHECK(num_buckets > 0 && num_buckets <= (int64_t)INT32_MAX,
              "bucket_sort_perm: num_buckets must be in 1..INT32_MAX, got ",
              num_buckets);
  int dtype = normalize_dtype_code(key.scalar_type());
  TORCH_CHECK(dtype != 2 && dtype != 3,
              "bucket_sort_perm: integer keys only");
  int64_t n = key.numel();
  TORCH_CHECK(bucket_ids.numel() == n, "bucket_ids length mismatch");
  if (n <= 1 || n > (int64_t)INT32_MAX) return py::none();
  auto dev = key.device();
  auto i64 = torch::dtype(torch::kInt64).device(dev);
  auto i32 = torch::dtype(torch::kInt32).device(dev);
  auto stream = current_stream();

  auto mm = torch::empty({2}, i64);
  hsk::key_minmax(key.data_ptr(), dtype, n,
                  (uint64_t*)mm.data_ptr<int64_t>(), stream);
  auto mm_host = mm.cpu();
  uint64_t kmin = (uint64_t)mm_host.data_ptr<int64_t>()[0];
  uint64_t range = (uint64_t)mm_host.data_ptr<int64_t>()[1] - kmin;
  int bbits = bit_length_u64((uint64_t)num_buckets - 1);
  int kbits = bit_length_u64(range);
  if (kbits + bbits > 64) return py::none();
  // the bucket field starts on a byte boundary so that it shares no
  // radix digit with the key, unless only the tight layout fits 64 bits
  int shift = (kbits + 7) / 8 * 8;
  if (shift + bbits > 64) shift = 64 - bbits;
  uint64_t low_mask = kbits ? ~0ull >> (64 - kbits) : 0;
  // varying bits, from the ranges alone: no reduce over the composite
  uint64_t mask = low_mask;
  if (bbits) mask |= (~0ull >> (64 - bbits)) << shift;

  auto comp = torch::empty({n}, i64);
  auto tmp_comp = torch::empty({n}, i64);
  auto perm = torch::empty({n}, i32);
  auto tmp_perm = torch::empty({n}, i32);
  auto hist = torch::empty({hsk::radix_sort_hist_size(n)}, i32);
  hsk::compose_bucket_key(key.data_ptr(), dtype,
                          bucket_ids.data_ptr<int32_t>(), kmin, shift,
                          (uint64_t*)comp.data_ptr<int64_t>(), n, stream);
  if (hsk::radix_sort_index32((uint64_t*)comp.data_ptr<int64_t>(),
                              perm.data_ptr<int32_t>(),
                              (uint64_t*)tmp_comp.data_ptr<int64_t>(),
                              tmp_perm.data_ptr<int32_t>(),
                              (uint32_t*)hist.data_ptr<int32_t>(), mask, n,
                              stream)) {
    std::swap(comp, tmp_comp);
    std::swap(perm, tmp_perm);
  }
  auto sorted = (const uint64_t*)comp.data_ptr<int64_t>();
  auto seg = torch::empty({num_buckets + 1}, i64);
  hsk::bucket_seg_offsets(sorted, n, shift, (int32_t)num_buckets,
                          seg.data_ptr<int64_t>(), stream);
  auto sorted_key = torch::empty_like(key);
  hsk::restore_key(sorted, low_mask, kmin, dtype, sorted_key.data_ptr(), n,
                   stream);
  return py::make_tuple(perm, sorted_key, seg.cpu());
}

// The group-by kernels read 16-byte vectors: a contiguous view that
// starts mid-allocation (a slice) is copied to an aligned buffer.
torch::Tensor aligned16(torch::Tensor t) {
  if (t.numel() > 0 && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 != 0)
    return t.clone();
  return t;
}

// Group offsets of adjacent equal rows: int64 [n_groups + 1].  keys: 1..8
// normalized u64 columns (int64-encoded); masks: empty, or parallel to
// keys with empty tensors for columns without nulls.
torch::Tensor group_offsets(std::vector<torch::Tensor> keys,
                            std::vector<torch::Tensor> masks) {
  TORCH_CHECK(!keys.empty() && keys.size() <= 8, "1..8 key columns");
  TORCH_CHECK(masks.empty() || masks.size() == keys.size(),
              "masks must be empty or parallel to keys");
  int64_t n = keys[0].numel();
  auto dev = keys[0].device();
  auto opts = torch::dtype(torch::kInt64).device(dev);
  if (n == 0) return torch::zeros({1}, opts);
  std::vector<torch::Tensor> held;
  const uint64_t* kptr[8] = {nullptr};
  const uint8_t* mptr[8] = {nullptr};
  for (size_t c = 0; c < keys.size(); ++c) {
    check_cuda(keys[c], "key");
    TORCH_CHECK(keys[c].scalar_type() == torch::kInt64,
                "keys must be normalized int64");
    TORCH_CHECK(keys[c].numel() == n, "key column length mismatch");
    held.push_back(aligned16(keys[c]));
    kptr[c] = (const uint64_t*)held.back().data_ptr<int64_t>();
    if (!masks.empty() && masks[c].numel() > 0) {
      check_cuda(masks[c], "mask");
      TORCH_CHECK(masks[c].numel() == n, "mask length mismatch");
      TORCH_CHECK(masks[c].scalar_type() == torch::kBool ||
                      masks[c].scalar_type() == torch::kUInt8,
                  "mask must be bool/uint8");
      held.push_back(aligned16(masks[c]));
      mptr[c] = (const uint8_t*)held.back().data_ptr();
    }
  }
  auto stream = current_stream();
  int64_t tile = hsk::group_tile_size();
  int64_t n_tiles = (n + tile - 1) / tile;
  auto tile_counts = torch::empty({n_tiles}, opts);
  hsk::group_offsets_count(kptr, mptr, (int)keys.size(), n,
                           tile_counts.data_ptr<int64_t>(), stream);
  auto tile_offsets = torch::empty({n_tiles}, opts);
  auto total = torch::empty({1}, opts);
  hsk::exclusive_scan_i64(tile_counts.data_ptr<int64_t>(),
                          tile_offsets.data_ptr<int64_t>(), n_tiles,
                          total.data_ptr<int64_t>(), stream);
  int64_t n_groups = total.cpu().item<int64_t>();
  auto out = torch::empty({n_groups + 1}, opts);
  hsk::group_offsets_emit(kptr, mptr, (int)keys.size(), n,
                          tile_offsets.data_ptr<int64_t>(),
                          total.data_ptr<int64_t>(), out.data_ptr<int64_t>(),
                          stream);
  return out;
}

// Fused segmented reduce: (sum, min, max, count) per group; want is a
// bit set (1 sum, 2 min, 4 max) — a tensor not asked for comes back
// empty.  count is always computed.  valid: empty = no nulls.
std::vector<torch::Tensor> segmented_reduce(torch::Tensor values,
                                            torch::Tensor valid,
                                            torch::Tensor offsets,
                                            int64_t want) {
  check_cuda(values, "values");
  int dtype;
  switch (values.scalar_type()) {
    case torch::kInt64: dtype = 0; break;
    case torch::kInt32: dtype = 1; break;
    case torch::kFloat64: dtype = 2; break;
    case torch::kFloat32: dtype = 3; break;
    default:
      TORCH_CHECK(false, "segmented_reduce: values must be int32, int64, "
                         "float32 or float64");
  }
  bool is_float = dtype >= 2;
  auto dev = values.device();
  int64_t n = values.numel();
  auto off_d = offsets.to(dev, torch::kInt64).contiguous();
  TORCH_CHECK(off_d.numel() >= 1, "offsets must have n_groups + 1 entries");
  int64_t n_groups = off_d.numel() - 1;
  auto i64 = torch::dtype(torch::kInt64).device(dev);
  auto sum_opts = is_float ? torch::dtype(torch::kFloat64).device(dev) : i64;
  // zero-filled: a group the kernel never closes (possible only with
  // malformed offsets) reads as empty
  auto sums = torch::zeros({(want & 1) ? n_groups : 0}, sum_opts);
  auto mins = torch::zeros({(want & 2) ? n_groups : 0}, values.options());
  auto maxs = torch::zeros({(want & 4) ? n_groups : 0}, values.options());
  auto counts = torch::zeros({n_groups}, i64);
  if (n == 0 || n_groups == 0) return {sums, mins, maxs, counts};
  values = aligned16(values);
  const uint8_t* vptr = nullptr;
  if (valid.numel() > 0) {
    check_cuda(valid, "valid");
    TORCH_CHECK(valid.numel() == n, "valid length mismatch");
    TORCH_CHECK(valid.scalar_type() == torch::kBool ||
                    valid.scalar_type() == torch::kUInt8,
                "valid must be bool/uint8");
    valid = aligned16(valid);
    vptr = (const uint8_t*)valid.data_ptr();
  }
  int64_t tile = hsk::group_tile_size();
  int64_t n_tiles = (n + tile - 1) / tile;
  auto tile_groups = torch::empty({n_tiles + 1}, i64);
  auto partials =
      torch::empty({4 * hsk::segmented_reduce_num_blocks(n)}, i64);
  hsk::segmented_reduce(values.data_ptr(), dtype, vptr,
                        off_d.data_ptr<int64_t>(), n, n_groups,
                        (want & 1) ? sums.data_ptr() : nullptr,
                        (want & 2) ? mins.data_ptr() : nullptr,
                        (want & 4) ? maxs.data_ptr() : nullptr,
                        counts.data_ptr<int64_t>(),
                        tile_groups.data_ptr<int64_t>(),
                        partials.data_ptr<int64_t>(), current_stream());
  return {sums, mins, maxs, counts};
}

int64_t group_tile_size() { return hsk::group_tile_size(); }

// Rows of the k smallest u64 keys (int64-encoded), ascending row index;
// valid: empty = all rows.  The one host read is the output length.
torch::Tensor topk_rows(torch::Tensor keys, int64_t k, torch::Tensor valid,
                        bool keep_ties) {
  check_cuda(keys, "keys");
  TORCH_CHECK(keys.scalar_type() == torch::kInt64,
              "keys must be normalized int64");
  int64_t n = keys.numel();
  auto opts = torch::dtype(torch::kInt64).device(keys.device());
  if (n == 0 || k <= 0) return torch::empty({0}, opts);
  if (k > n) k = n;
  keys = aligned16(keys);
  const uint8_t* vptr = nullptr;
  if (valid.numel() > 0) {
    check_cuda(valid, "valid");
    TORCH_CHECK(valid.numel() == n, "valid length mismatch");
    TORCH_CHECK(valid.scalar_type() == torch::kBool ||
                    valid.scalar_type() == torch::kUInt8,
                "valid must be bool/uint8");
    valid = aligned16(valid);
    vptr = (const uint8_t*)valid.data_ptr();
  }
  auto stream = current_stream();
  auto scratch = torch::zeros({hsk::topk_scratch_size(n)}, opts);
  const uint64_t* kp = (const uint64_t*)keys.data_ptr<int64_t>();
  int64_t* d_total = hsk::topk_select(kp, vptr, n, k, keep_ties,
                                      scratch.data_ptr<int64_t>(), stream);
  int64_t idx = d_total - scratch.data_ptr<int64_t>();
  int64_t n_out = scratch.narrow(0, idx, 1).cpu().item<int64_t>();
  TORCH_CHECK(n_out >= 0 && n_out <= n, "topk_rows: bad output length");
  auto out = torch::empty({n_out}, opts);
  hsk::topk_emit(kp, vptr, n, scratch.data_ptr<int64_t>(),
                 out.data_ptr<int64_t>(), n_out, stream);
  return out;
}

int64_t topk_tile_size() { return hsk::topk_tile_size(); }

// All bucket files of one batch in one GIL-released call
// (bucket_writer.h).  cols: 1-D contiguous int32/int64/float32/float64
// tensors, all on one device or all on the host; stats: per (file, column)
// PLAIN min/max bytes, file-major; ring: pinned uint8 staging of the
// caller and stream0/stream1 the raw handles of two torch streams (device
// batches; all three ignored for host batches).  Returns (sizes,
// mtimes_ns, payload starts, payload ends), the last two file-major.
std::tuple<std::vector<int64_t>, std::vector<int64_t>, std::vector<int64_t>,
           std::vector<int64_t>>
write_bucket_files(std::vector<torch::Tensor> cols,
                   std::vector<std::string> names,
                   std::vector<std::string> paths,
                   std::vector<int64_t> row_lo, std::vector<int64_t> row_hi,
                   std::vector<std::string> mins,
                   std::vector<std::string> maxs, torch::Tensor ring,
                   int64_t chunk_bytes, int64_t writer_threads,
                   int64_t stream0, int64_t stream1, bool timing) {
  TORCH_CHECK(!cols.empty() && cols.size() == names.size(),
              "write_bucket_files: columns and names must be parallel");
  TORCH_CHECK(paths.size() == row_lo.size() && paths.size() == row_hi.size(),
              "write_bucket_files: paths and row ranges must be parallel");
  TORCH_CHECK(mins.size() == paths.size() * cols.size() &&
                  maxs.size() == mins.size(),
              "write_bucket_files: one (min, max) per file and column");
  TORCH_CHECK(chunk_bytes > 0 && writer_threads >= 1 && writer_threads <= 15,
              "write_bucket_files: chunk_bytes > 0, 1 <= threads <= 15");
  const bool on_device = cols[0].is_cuda();
  const int64_t n = cols[0].numel();
  std::vector<hsw::Column> wc;
  for (size_t c = 0; c < cols.size(); c++) {
    const torch::Tensor& t = cols[c];
    TORCH_CHECK(t.dim() == 1 && t.is_contiguous() && t.numel() == n &&
                    t.device() == cols[0].device(),
                "write_bucket_files: columns must be 1-D, contiguous, of "
                "one length and on one device");
    int ptype;
    switch (t.scalar_type()) {
      case torch::kInt64: ptype = hsw::T_INT64; break;
      case torch::kInt32: ptype = hsw::T_INT32; break;
      case torch::kFloat64: ptype = hsw::T_DOUBLE; break;
      case torch::kFloat32: ptype = hsw::T_FLOAT; break;
      default:
        TORCH_CHECK(false, "write_bucket_files: unsupported column dtype");
    }
    wc.push_back({t.data_ptr(), (int)t.element_size(), ptype, names[c]});
  }
  std::vector<hsw::FileJob> jobs;
  for (size_t f = 0; f < paths.size(); f++) {
    TORCH_CHECK(0 <= row_lo[f] && row_lo[f] < row_hi[f] && row_hi[f] <= n,
                "write_bucket_files: row range of file ", f,
                " is empty or outside the batch");
    jobs.push_back({paths[f], row_lo[f], row_hi[f]});
  }
  std::vector<std::pair<std::string, std::string>> stats;
  for (size_t i = 0; i < mins.size(); i++)
    stats.emplace_back(std::move(mins[i]), std::move(maxs[i]));

  hsw::Options opt;
  opt.chunk_bytes = (size_t)chunk_bytes;
  opt.writer_threads = (int)writer_threads;
  opt.device_source = on_device;
  opt.timing = timing;
  std::vector<hsw::FileResult> res;
  if (on_device) {
    TORCH_CHECK(ring.device().is_cpu() && ring.is_pinned() &&
                    ring.is_contiguous() &&
                    ring.scalar_type() == torch::kUInt8 &&
                    ring.numel() >= chunk_bytes,
                "write_bucket_files: ring must be a pinned uint8 tensor of "
                "at least one chunk");
    // the caller has made the columns' device current
    // two streams of torch's pool, handed in by the caller: the process
    // opens few hardware queues, so none is created here
    opt.streams[0] = reinterpret_cast<hipStream_t>(stream0);
    opt.streams[1] = reinterpret_cast<hipStream_t>(stream1);
    opt.ring = ring.data_ptr();
    opt.ring_bytes = (size_t)ring.numel();
    hipEvent_t start = nullptr;
    TORCH_CHECK(hipEventCreateWithFlags(&start, hipEventDisableTiming) ==
                    hipSuccess,
                "write_bucket_files: hipEventCreate failed");
    // the copies follow whatever the caller's stream has queued so far
    hipError_t e = hipEventRecord(start, current_stream());
    opt.start_event = start;
    std::string err;
    if (e != hipSuccess) {
      err = std::string("hipEventRecord: ") + hipGetErrorString(e);
    } else {
      py::gil_scoped_release rel;
      try {
        res = hsw::write_bucket_files(wc, jobs, stats, opt);
      } catch (const std::exception& ex) {
        err = ex.what();
      }
    }
    (void)hipEventDestroy(start);
    TORCH_CHECK(err.empty(), err);
  } else {
    py::gil_scoped_release rel;
    res = hsw::write_bucket_files(wc, jobs, stats, opt);
  }
  std::vector<int64_t> sizes, mtimes, starts, ends;
  for (const hsw::FileResult& r : res) {
    sizes.push_back(r.size);
    mtimes.push_back(r.mtime_ns);
    starts.insert(starts.end(), r.payload_start.begin(),
                  r.payload_start.end());
    ends.insert(ends.end(), r.payload_end.begin(), r.payload_end.end());
  }
  return {sizes, mtimes, starts, ends};
}

}  // namespace

// out-of-namespace impl so the two-phase select is a single public symbol
torch::Tensor select_range_u64_pub(torch::Tensor keys, int64_t lo,
                                   int64_t hi, bool lo_incl, bool hi_incl) {
  TORCH_CHECK(keys.is_cuda() && keys.is_contiguous(), "keys");
  auto n = keys.numel();
  auto opts = torch::dtype(torch::kInt64).device(keys.device());
  if (n == 0) return torch::empty({0}, opts);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  int64_t nb = hsk::select_num_blocks(n);
  auto bcounts = torch::empty({nb}, opts);
  auto total = torch::empty({1}, opts);
  // lo/hi arrive already u64-normalized (int64-encoded); the kernel
  // compares raw u64 bits, so reinterpret without remapping
  uint64_t ulo = (uint64_t)lo;
  uint64_t uhi = (uint64_t)hi;
  // phase 1: count + scan
  hsk::select_range_count((const uint64_t*)keys.data_ptr<int64_t>(), n, ulo,
                          uhi, lo_incl, hi_incl,
                          bcounts.data_ptr<int64_t>(),
                          total.data_ptr<int64_t>(), stream);
  int64_t n_out = total.cpu().item<int64_t>();
  auto out = torch::empty({n_out}, opts);
  if (n_out > 0) {
    hsk::select_range_emit((const uint64_t*)keys.data_ptr<int64_t>(), n, ulo,
                           uhi, lo_incl, hi_incl,
                           bcounts.data_ptr<int64_t>(),
                           out.data_ptr<int64_t>(), stream);
  }
  return out;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("murmur3_bucket", &murmur3_bucket, "Spark-compatible murmur3 bucket",
        py::arg("keys"), py::arg("num_buckets"),
        py::arg("masks") = std::vector<torch::Tensor>{});
  m.def("normalize_key", &normalize_key, "order-preserving u64 key",
        py::arg("vals"), py::arg("canonical") = false,
        py::arg("descending") = false);
  m.def("radix_sort_pairs", &radix_sort_pairs, "stable LSD radix sort");
  m.def("radix_sort_plan", &radix_sort_plan,
        "pass plan of the radix sort for a varying-bit mask: "
        "(radix, [shifts])");
  m.def("exclusive_scan", &exclusive_scan,
        "device-wide exclusive scan of an int64 tensor: (out, total)");
  m.def("merge_join", &merge_join, "segmented sorted merge join",
        py::arg("lkeys"), py::arg("rkeys"), py::arg("lseg"), py::arg("rseg"),
        py::arg("mode") = 0);
  m.def("select_range_u64", &select_range_u64_pub, "range filter compaction");
  m.def("isin_sorted", &isin_sorted, "sorted-set membership");
  m.def("segmented_minmax", &segmented_minmax, "per-segment min/max");
  m.def("bloom_build", &bloom_build, "bloom filter build");
  m.def("bloom_probe", &bloom_probe, "bloom filter probe");
  m.def("bloom_probe_many", &bloom_probe_many,
        "K9 device sketch-predicate probe over per-file filters");
  m.def("zorder_key", &zorder_key, "z-order bit interleave");
  m.def("gather_rows", &gather_rows,
        "row gather by an int64 or int32 index");
  m.def("bucket_sort_perm", &bucket_sort_perm,
        "fused (bucket, integer key) sort: (perm int32, sorted key column, "
        "seg) or None when the key range is too wide");
  m.def("copy_unaligned", &copy_unaligned,
        "device parquet page decode (unaligned copy)");
  m.def("run_merge_perm", &run_merge_perm,
        "segmented two-sorted-run merge permutation");
  m.def("group_offsets", &group_offsets,
        "offsets of adjacent equal-key runs: int64 [n_groups + 1]",
        py::arg("keys"), py::arg("masks") = std::vector<torch::Tensor>{});
  m.def("segmented_reduce", &segmented_reduce,
        "fused per-group (sum, min, max, count); want bits 1/2/4");
  m.def("write_bucket_files", &write_bucket_files,
        "write every bucket file of a batch: chunked D2H through a pinned "
        "ring into pwrite (host batches: pwrite from the columns)");
  m.def("group_tile_size", &group_tile_size,
        "rows per tile of the group-by kernels");
  m.def("topk_rows", &topk_rows,
        "rows of the k smallest keys by radix select, ascending row index",
        py::arg("keys"), py::arg("k"), py::arg("valid"),
        py::arg("keep_ties") = false);
  m.def("topk_tile_size", &topk_tile_size,
        "rows per tile of the top-k kernels");
  m.def("snappy_decompress", &snappy_decompress,
        "device snappy raw-block page decompression; returns status");
  m.def("decode_def_levels", &decode_def_levels,
        "host RLE-hybrid def-level decode -> bool validity");
  m.def("parse_rle_runs_batch", &parse_rle_runs_batch,
        py::call_guard<py::gil_scoped_release>(),
        "batched RLE-hybrid run parse over many pages");
  m.def("parse_rle_runs", &parse_rle_runs,
        py::call_guard<py::gil_scoped_release>(),
        "host parse of an RLE/bit-packed hybrid run table");
  m.def("parse_byte_arrays", &parse_byte_arrays,
        py::call_guard<py::gil_scoped_release>(),
        "host PLAIN byte-array page parse -> (offsets, bytes)");
  m.def("host_memcpy", &host_memcpy,
        "GIL-released buffer -> cpu-u8-tensor memcpy");
  m.def("rle_decode", &rle_decode,
        "device RLE/bit-packed dictionary-index decode");
}
