// CDNA4 (gfx950 / MI355X) group-by kernels for hyperspace_amd: group
// offsets of adjacent equal keys and the fused segmented reduce over them.
//
// Both ops divide the work over ROWS in fixed tiles of AG_TILE rows (256
// threads, wave64), never over groups, so n groups of one row and one
// group of n rows run through the same code at the same rate.
//
//   group_offsets     count pass (heads per tile) -> exclusive_scan_i64 ->
//                     emit pass (ballot ranks inside the tile), the shape
//                     of select_range_count / select_range_emit.
//   segmented_reduce  one launch reads values (+ validity) once and gives
//                     sum, min, max and valid-count of every group.  A
//                     block walks a contiguous range of tiles and carries
//                     the open group in registers; a group that leaves the
//                     block is finished by a small ordered fix-up pass over
//                     per-block partials.  No atomics anywhere: float sums
//                     are bitwise reproducible from run to run.
//
// Streaming, memory-bound: every global load of values is a 16-byte
// lane-contiguous vector (1 KiB per wave instruction) staged through LDS
// into the 8-rows-per-thread blocked layout the segmented scan needs.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "kernels.h"

namespace hsk {

namespace {

constexpr int AG_THREADS = 256;
constexpr int AG_WAVES = AG_THREADS / 64;
constexpr int AG_RPT = 8;                       // rows per thread
constexpr int AG_TILE = AG_THREADS * AG_RPT;    // 2048 rows per tile
constexpr int AG_MAX_BLOCKS = 2048;             // 256 CUs x 8 blocks/CU
constexpr int AG_MAX_KEYS = 8;

static inline int64_t ag_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------------------
// group_offsets
// ---------------------------------------------------------------------------

struct GroupKeys {
  const uint64_t* k[AG_MAX_KEYS];
  const uint8_t* m[AG_MAX_KEYS];  // validity bytes or nullptr
  int n_cols;
};

__device__ __forceinline__ bool ag_differ(bool va, uint64_t ka, bool vb,
                                          uint64_t kb) {
  // (null flag, key) pairs; the stored key of a null row is ignored
  return (va != vb) || (va && ka != kb);
}

// Head flags of rows r and r + 1 (r even, one 16-byte key load per
// column).  The row before r comes from the lane below; lane 0 of a wave
// reads it from memory.  Every lane of the wave must call this.
__device__ __forceinline__ void ag_pair_heads(const GroupKeys& gk, int64_t r,
                                              int64_t n, int lane, bool& h0,
                                              bool& h1) {
  bool d0 = false, d1 = false;
  for (int c = 0; c < gk.n_cols; c++) {
    const uint64_t* kp = gk.k[c];
    const uint8_t* mp = gk.m[c];
    uint64_t k0 = 0, k1 = 0;
    int v0 = 1, v1 = 1;
    if (r + 1 < n) {
      ulonglong2 kk = *reinterpret_cast<const ulonglong2*>(kp + r);
      k0 = kk.x;
      k1 = kk.y;
      if (mp != nullptr) {
        uchar2 mm = *reinterpret_cast<const uchar2*>(mp + r);
        v0 = mm.x != 0;
        v1 = mm.y != 0;
      }
    } else if (r < n) {
      k0 = kp[r];
      if (mp != nullptr) v0 = mp[r] != 0;
    }
    uint64_t kprev = __shfl_up((unsigned long long)k1, 1);
    int vprev = __shfl_up(v1, 1);
    if (lane == 0 && r > 0 && r < n) {
      kprev = kp[r - 1];
      vprev = mp != nullptr ? (mp[r - 1] != 0) : 1;
    }
    d0 |= ag_differ(vprev != 0, kprev, v0 != 0, k0);
    d1 |= ag_differ(v0 != 0, k0, v1 != 0, k1);
  }
  h0 = (r < n) && (r == 0 || d0);
  h1 = (r + 1 < n) && d1;
}

constexpr int AG_PAIR_ITERS = AG_TILE / (AG_THREADS * 2);  // 4

__global__ __launch_bounds__(AG_THREADS) void k_group_count(
    GroupKeys gk, int64_t n, int64_t* __restrict__ tile_counts) {
  __shared__ int s_cnt[AG_WAVES];
  int lane = threadIdx.x & 63;
  int wave = threadIdx.x >> 6;
  int64_t ts = (int64_t)blockIdx.x * AG_TILE;
  int cnt = 0;
#pragma unroll
  for (int it = 0; it < AG_PAIR_ITERS; it++) {
    int64_t r = ts + (int64_t)(it * AG_THREADS + threadIdx.x) * 2;
    bool h0, h1;
    ag_pair_heads(gk, r, n, lane, h0, h1);
    cnt += (int)h0 + (int)h1;
  }
  for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d);
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < AG_WAVES; w++) t += s_cnt[w];
    tile_counts[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(AG_THREADS) void k_group_emit(
    GroupKeys gk, int64_t n, const int64_t* __restrict__ tile_offsets,
    const int64_t* __restrict__ total, int64_t* __restrict__ out) {
  __shared__ int s_cnt[AG_PAIR_ITERS * AG_WAVES];
  int lane = threadIdx.x & 63;
  int wave = threadIdx.x >> 6;
  int64_t ts = (int64_t)blockIdx.x * AG_TILE;
  bool h0[AG_PAIR_ITERS], h1[AG_PAIR_ITERS];
  int rank[AG_PAIR_ITERS];
  unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int it = 0; it < AG_PAIR_ITERS; it++) {
    int64_t r = ts + (int64_t)(it * AG_THREADS + threadIdx.x) * 2;
    ag_pair_heads(gk, r, n, lane, h0[it], h1[it]);
    unsigned long long b0 = __ballot(h0[it]);
    unsigned long long b1 = __ballot(h1[it]);
    rank[it] = __popcll(b0 & below) + __popcll(b1 & below);
    if (lane == 0) s_cnt[it * AG_WAVES + wave] = __popcll(b0) + __popcll(b1);
  }
  __syncthreads();
  int64_t base = tile_offsets[blockIdx.x];
#pragma unroll
  for (int it = 0; it < AG_PAIR_ITERS; it++) {
    int pre = 0;
    for (int j = 0; j < it * AG_WAVES + wave; j++) pre += s_cnt[j];
    int64_t r = ts + (int64_t)(it * AG_THREADS + threadIdx.x) * 2;
    int64_t o = base + pre + rank[it];
    if (h0[it]) out[o++] = r;
    if (h1[it]) out[o] = r + 1;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[total[0]] = n;
}

static GroupKeys make_group_keys(const uint64_t* const* keys,
                                 const uint8_t* const* masks, int n_cols) {
  GroupKeys gk{};
  gk.n_cols = n_cols < AG_MAX_KEYS ? n_cols : AG_MAX_KEYS;
  for (int c = 0; c < gk.n_cols; c++) {
    gk.k[c] = keys[c];
    gk.m[c] = masks != nullptr ? masks[c] : nullptr;
  }
  return gk;
}

// ---------------------------------------------------------------------------
// segmented_reduce
// ---------------------------------------------------------------------------

// Order-preserving u64 image of a value (the order normalize_key defines,
// so float min/max agree with the sort: -NaN < -inf < -0.0 < +0.0 < +inf <
// +NaN) and its inverse.
template <typename T>
struct Ord;
template <>
struct Ord<int64_t> {
  __device__ static uint64_t key(int64_t x) {
    return (uint64_t)x ^ 0x8000000000000000ull;
  }
  __device__ static int64_t val(uint64_t k) {
    return (int64_t)(k ^ 0x8000000000000000ull);
  }
};
template <>
struct Ord<int32_t> {
  __device__ static uint64_t key(int32_t x) {
    return (uint64_t)(int64_t)x ^ 0x8000000000000000ull;
  }
  __device__ static int32_t val(uint64_t k) {
    return (int32_t)(int64_t)(k ^ 0x8000000000000000ull);
  }
};
template <>
struct Ord<double> {
  __device__ static uint64_t key(double x) {
    uint64_t b = (uint64_t)__double_as_longlong(x);
    return b ^ ((b >> 63) ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull);
  }
  __device__ static double val(uint64_t k) {
    uint64_t b = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
    return __longlong_as_double((long long)b);
  }
};
template <>
struct Ord<float> {
  __device__ static uint64_t key(float x) {
    uint32_t b = __float_as_uint(x);
    return (uint64_t)(b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u));
  }
  __device__ static float val(uint64_t k) {
    uint32_t k32 = (uint32_t)k;
    uint32_t b = (k32 >> 31) ? (k32 ^ 0x80000000u) : ~k32;
    return __uint_as_float(b);
  }
};

// integer sums wrap (two's complement) -> accumulate unsigned
template <typename T>
using SumT = typename std::conditional<std::is_floating_point<T>::value,
                                       double, unsigned long long>::type;

template <typename S>
struct Acc {
  S sum;
  unsigned long long mn, mx;  // Ord keys; meaningful when cnt > 0
  long long cnt;
};

template <typename S>
__device__ __forceinline__ Acc<S> acc_identity() {
  Acc<S> a;
  a.sum = (S)0;
  a.mn = 0xFFFFFFFFFFFFFFFFull;
  a.mx = 0ull;
  a.cnt = 0;
  return a;
}

// a covers earlier rows than b: the float order of additions is fixed
template <typename S>
__device__ __forceinline__ Acc<S> acc_combine(const Acc<S>& a,
                                              const Acc<S>& b) {
  Acc<S> r;
  r.sum = a.sum + b.sum;
  r.mn = a.mn < b.mn ? a.mn : b.mn;
  r.mx = a.mx > b.mx ? a.mx : b.mx;
  r.cnt = a.cnt + b.cnt;
  return r;
}

template <typename T, typename S>
__device__ __forceinline__ void acc_add(Acc<S>& a, T x) {
  uint64_t k = Ord<T>::key(x);
  if constexpr (std::is_floating_point<T>::value)
    a.sum += (S)x;
  else
    a.sum += (S)(long long)x;
  a.mn = k < a.mn ? k : a.mn;
  a.mx = k > a.mx ? k : a.mx;
  a.cnt += 1;
}

template <typename S>
__device__ __forceinline__ Acc<S> acc_shfl_up(const Acc<S>& a, int d) {
  Acc<S> r;
  r.sum = __shfl_up(a.sum, d);
  r.mn = __shfl_up(a.mn, d);
  r.mx = __shfl_up(a.mx, d);
  r.cnt = __shfl_up(a.cnt, d);
  return r;
}

template <typename S>
__device__ __forceinline__ Acc<S> acc_shfl_down(const Acc<S>& a, int d) {
  Acc<S> r;
  r.sum = __shfl_down(a.sum, d);
  r.mn = __shfl_down(a.mn, d);
  r.mx = __shfl_down(a.mx, d);
  r.cnt = __shfl_down(a.cnt, d);
  return r;
}

// Output arrays of one column; sum/min/max may be null (not asked for).
template <typename T>
struct SegOut {
  SumT<T>* sum;
  T* mn;
  T* mx;
  int64_t* cnt;
  int64_t n_groups;
};

// Per-block partials: aggregate of the block's rows ahead of its first
// group head (the whole block when it has none).
template <typename S>
struct SegPartials {
  S* sum;
  unsigned long long* mn;
  unsigned long long* mx;
  long long* cnt;
};

template <typename T>
__device__ __forceinline__ void seg_store(const SegOut<T>& o, int64_t g,
                                          const Acc<SumT<T>>& a) {
  if (g < 0 || g >= o.n_groups) return;  // only on malformed offsets
  if (o.sum != nullptr) o.sum[g] = a.sum;
  if (o.mn != nullptr) o.mn[g] = a.cnt > 0 ? Ord<T>::val(a.mn) : (T)0;
  if (o.mx != nullptr) o.mx[g] = a.cnt > 0 ? Ord<T>::val(a.mx) : (T)0;
  o.cnt[g] = a.cnt;
}

template <typename S>
__device__ __forceinline__ void part_store(const SegPartials<S>& p, int64_t b,
                                           const Acc<S>& a) {
  p.sum[b] = a.sum;
  p.mn[b] = a.mn;
  p.mx[b] = a.mx;
  p.cnt[b] = a.cnt;
}

// tile_g[k] = number of groups that start before row k * AG_TILE, for
// k = 0 .. n_tiles.  The groups whose head lies in tile k are
// [tile_g[k], tile_g[k + 1]).
__global__ void k_tile_groups(const int64_t* __restrict__ offsets,
                              int64_t n_groups, int64_t n_tiles,
                              int64_t* __restrict__ tile_g) {
  int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > n_tiles) return;
  int64_t target = k * AG_TILE;
  int64_t lo = 0, hi = n_groups;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (offsets[mid] < target)
      lo = mid + 1;
    else
      hi = mid;
  }
  tile_g[k] = lo;
}

template <typename T>
__global__ __launch_bounds__(AG_THREADS) void k_seg_reduce(
    const T* __restrict__ vals, const uint8_t* __restrict__ valid,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ tile_g,
    int64_t n, int64_t n_tiles, int64_t tiles_per_block, SegOut<T> out,
    SegPartials<SumT<T>> part) {
  using S = SumT<T>;
  using A = Acc<S>;
  constexpr int VEC = 16 / (int)sizeof(T);
  __shared__ __attribute__((aligned(16))) T s_vals[AG_TILE];
  __shared__ __attribute__((aligned(16))) uint8_t s_head[AG_TILE];
  __shared__ A s_wacc[AG_WAVES];
  __shared__ int s_wflag[AG_WAVES];
  __shared__ int s_wheads[AG_WAVES];

  int tid = threadIdx.x;
  int lane = tid & 63;
  int wave = tid >> 6;
  int64_t k0 = (int64_t)blockIdx.x * tiles_per_block;
  int64_t k1 = k0 + tiles_per_block < n_tiles ? k0 + tiles_per_block : n_tiles;
  int64_t g0 = tile_g[k0];
  A carry = acc_identity<S>();  // open group at the end of the last tile

  for (int64_t k = k0; k < k1; k++) {
    int64_t ts = k * AG_TILE;
    int64_t ga = tile_g[k], gb = tile_g[k + 1];

    // stage: coalesced 16-byte loads -> LDS, clear the head bytes
    *reinterpret_cast<unsigned long long*>(&s_head[tid * AG_RPT]) = 0ull;
#pragma unroll
    for (int it = 0; it < AG_TILE / (AG_THREADS * VEC); it++) {
      int p = (it * AG_THREADS + tid) * VEC;
      int64_t r = ts + p;
      if (r + VEC <= n) {
        *reinterpret_cast<uint4*>(&s_vals[p]) =
            *reinterpret_cast<const uint4*>(&vals[r]);
      } else {
        for (int e = 0; e < VEC; e++)
          s_vals[p + e] = (r + e < n) ? vals[r + e] : (T)0;
      }
    }
    __syncthreads();
    for (int64_t g = ga + tid; g < gb; g += AG_THREADS) {
      int64_t p = offsets[g] - ts;
      if (p >= 0 && p < AG_TILE) s_head[p] = 1;
    }
    __syncthreads();

    // this thread's 8 consecutive rows
    int64_t r8 = ts + (int64_t)tid * AG_RPT;
    unsigned long long hb =
        *reinterpret_cast<const unsigned long long*>(&s_head[tid * AG_RPT]);
    unsigned long long vb = 0x0101010101010101ull;
    if (valid != nullptr) {
      if (r8 + AG_RPT <= n) {
        vb = *reinterpret_cast<const unsigned long long*>(&valid[r8]);
      } else {
        vb = 0ull;
        for (int e = 0; e < AG_RPT; e++)
          if (r8 + e < n && valid[r8 + e] != 0) vb |= 1ull << (8 * e);
      }
    }
    int64_t left = n - r8;
    if (left <= 0)
      vb = 0ull;
    else if (left < AG_RPT)
      vb &= ~0ull >> (64 - 8 * (int)left);
    T x[AG_RPT];
#pragma unroll
    for (int i = 0; i < AG_RPT; i++) x[i] = s_vals[tid * AG_RPT + i];

    // pass 1: aggregate of the rows after this thread's last head
    A cur = acc_identity<S>();
    int nh = 0;
#pragma unroll
    for (int i = 0; i < AG_RPT; i++) {
      if ((hb >> (8 * i)) & 0xffull) {
        cur = acc_identity<S>();
        nh++;
      }
      if ((vb >> (8 * i)) & 0xffull) acc_add<T, S>(cur, x[i]);
    }

    // segmented inclusive scan over the wave, then over the 4 waves
    A inc = cur;
    int fl = nh > 0;
    int hc = nh;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      A o = acc_shfl_up(inc, d);
      int of = __shfl_up(fl, d);
      int oh = __shfl_up(hc, d);
      if (lane >= d) {
        if (!fl) inc = acc_combine(o, inc);
        fl |= of;
        hc += oh;
      }
    }
    A ex = acc_shfl_up(inc, 1);
    int exf = __shfl_up(fl, 1);
    int exh = __shfl_up(hc, 1);
    if (lane == 0) {
      ex = acc_identity<S>();
      exf = 0;
      exh = 0;
    }
    if (lane == 63) {
      s_wacc[wave] = inc;
      s_wflag[wave] = fl;
      s_wheads[wave] = hc;
    }
    __syncthreads();
    A c = carry;
    A cin_wave = carry;
    int hbase = 0, hbase_wave = 0;
#pragma unroll
    for (int w = 0; w < AG_WAVES; w++) {
      if (w == wave) {
        cin_wave = c;
        hbase_wave = hbase;
      }
      A wt = s_wacc[w];
      c = s_wflag[w] ? wt : acc_combine(c, wt);
      hbase += s_wheads[w];
    }
    carry = c;
    A cin = exf ? ex : acc_combine(cin_wave, ex);
    int hex = hbase_wave + exh;  // heads of this tile ahead of this thread

    // pass 2: close groups at their successor's head
    cur = cin;
    int kk = hex;
#pragma unroll
    for (int i = 0; i < AG_RPT; i++) {
      if ((hb >> (8 * i)) & 0xffull) {
        if (kk == 0 && ga == g0)
          part_store(part, (int64_t)blockIdx.x, cur);  // block's first head
        else
          seg_store(out, ga + kk - 1, cur);
        cur = acc_identity<S>();
        kk++;
      }
      if ((vb >> (8 * i)) & 0xffull) acc_add<T, S>(cur, x[i]);
    }
    __syncthreads();  // LDS is restaged by the next tile
  }

  if (tid == 0) {
    int64_t gl = tile_g[k1];
    if (gl == g0)
      part_store(part, (int64_t)blockIdx.x, carry);  // no head in the block
    else
      seg_store(out, gl - 1, carry);  // partial if the group goes on
  }
}

// Ordered fix-up: one wave per block b whose last group starts in b and
// runs on into later blocks.  Lanes fold contiguous chunks of the later
// blocks' partials in block order, then a fixed shuffle tree joins the
// lanes left to right — same order every run.
template <typename T>
__global__ __launch_bounds__(AG_THREADS) void k_seg_fixup(
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ tile_g,
    int64_t n, int64_t n_groups, int64_t n_tiles, int64_t tiles_per_block,
    int64_t n_blocks, SegOut<T> out, SegPartials<SumT<T>> part) {
  using S = SumT<T>;
  using A = Acc<S>;
  int lane = threadIdx.x & 63;
  int64_t b = (int64_t)blockIdx.x * AG_WAVES + (threadIdx.x >> 6);
  if (b >= n_blocks) return;  // wave-uniform
  int64_t k0 = b * tiles_per_block;
  int64_t k1 = k0 + tiles_per_block < n_tiles ? k0 + tiles_per_block : n_tiles;
  int64_t rows_per_block = tiles_per_block * AG_TILE;
  int64_t r1 = k1 * AG_TILE;
  if (r1 >= n) return;
  if (tile_g[k1] <= tile_g[k0]) return;  // group not started here
  int64_t g = tile_g[k1] - 1;
  int64_t e = offsets[g + 1];  // g + 1 <= n_groups
  if (e > n) e = n;
  if (e <= r1) return;  // ends with the block
  int64_t bl = (e - 1) / rows_per_block;
  if (bl > n_blocks - 1) bl = n_blocks - 1;
  int64_t span = bl - b;
  int64_t chunk = (span + 63) / 64;
  int64_t j0 = b + 1 + lane * chunk;
  int64_t j1 = j0 + chunk < bl + 1 ? j0 + chunk : bl + 1;
  A a = acc_identity<S>();
  for (int64_t j = j0; j < j1; j++) {
    A p;
    p.sum = part.sum[j];
    p.mn = part.mn[j];
    p.mx = part.mx[j];
    p.cnt = part.cnt[j];
    a = acc_combine(a, p);
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    A o = acc_shfl_down(a, d);
    if ((lane & (2 * d - 1)) == 0) a = acc_combine(a, o);
  }
  if (lane == 0) {
    A own;
    own.cnt = out.cnt[g];
    own.sum = out.sum != nullptr ? out.sum[g] : (S)0;
    own.mn = (out.mn != nullptr && own.cnt > 0) ? Ord<T>::key(out.mn[g])
                                                : 0xFFFFFFFFFFFFFFFFull;
    own.mx = (out.mx != nullptr && own.cnt > 0) ? Ord<T>::key(out.mx[g])
                                                : 0ull;
    seg_store(out, g, acc_combine(own, a));
  }
}

static inline int64_t seg_tiles_per_block(int64_t n_tiles) {
  return n_tiles > AG_MAX_BLOCKS ? ag_cdiv(n_tiles, AG_MAX_BLOCKS) : 1;
}

template <typename T>
static void seg_reduce_launch(const void* vals, const uint8_t* valid,
                              const int64_t* offsets, int64_t n,
                              int64_t n_groups, void* sums, void* mins,
                              void* maxs, int64_t* counts, int64_t* tile_groups,
                              int64_t* partials, hipStream_t stream) {
  using S = SumT<T>;
  int64_t n_tiles = ag_cdiv(n, AG_TILE);
  int64_t tpb = seg_tiles_per_block(n_tiles);
  int64_t nb = ag_cdiv(n_tiles, tpb);
  SegOut<T> out{(S*)sums, (T*)mins, (T*)maxs, counts, n_groups};
  SegPartials<S> part{(S*)partials, (unsigned long long*)(partials + nb),
                      (unsigned long long*)(partials + 2 * nb),
                      (long long*)(partials + 3 * nb)};
  hipLaunchKernelGGL(k_tile_groups, dim3((unsigned)ag_cdiv(n_tiles + 1, 256)),
                     dim3(256), 0, stream, offsets, n_groups, n_tiles,
                     tile_groups);
  hipLaunchKernelGGL((k_seg_reduce<T>), dim3((unsigned)nb), dim3(AG_THREADS),
                     0, stream, (const T*)vals, valid, offsets,
                     (const int64_t*)tile_groups, n, n_tiles, tpb, out, part);
  if (nb > 1)
    hipLaunchKernelGGL((k_seg_fixup<T>),
                       dim3((unsigned)ag_cdiv(nb, AG_WAVES)), dim3(AG_THREADS),
                       0, stream, offsets, (const int64_t*)tile_groups, n,
                       n_groups, n_tiles, tpb, nb, out, part);
}

}  // namespace

int64_t group_tile_size() { return AG_TILE; }

void group_offsets_count(const uint64_t* const* keys,
                         const uint8_t* const* masks, int n_cols, int64_t n,
                         int64_t* tile_counts, hipStream_t stream) {
  if (n == 0) return;
  GroupKeys gk = make_group_keys(keys, masks, n_cols);
  hipLaunchKernelGGL(k_group_count, dim3((unsigned)ag_cdiv(n, AG_TILE)),
                     dim3(AG_THREADS), 0, stream, gk, n, tile_counts);
}

void group_offsets_emit(const uint64_t* const* keys,
                        const uint8_t* const* masks, int n_cols, int64_t n,
                        const int64_t* tile_offsets, const int64_t* total,
                        int64_t* out, hipStream_t stream) {
  if (n == 0) return;
  GroupKeys gk = make_group_keys(keys, masks, n_cols);
  hipLaunchKernelGGL(k_group_emit, dim3((unsigned)ag_cdiv(n, AG_TILE)),
                     dim3(AG_THREADS), 0, stream, gk, n, tile_offsets, total,
                     out);
}

int64_t segmented_reduce_num_blocks(int64_t n) {
  int64_t n_tiles = ag_cdiv(n, AG_TILE);
  if (n_tiles < 1) return 1;
  return ag_cdiv(n_tiles, seg_tiles_per_block(n_tiles));
}

void segmented_reduce(const void* vals, int dtype, const uint8_t* valid,
                      const int64_t* offsets, int64_t n, int64_t n_groups,
                      void* sums, void* mins, void* maxs, int64_t* counts,
                      int64_t* tile_groups, int64_t* partials,
                      hipStream_t stream) {
  if (n == 0 || n_groups == 0) return;
  switch (dtype) {
    case 0:
      seg_reduce_launch<int64_t>(vals, valid, offsets, n, n_groups, sums, mins,
                                 maxs, counts, tile_groups, partials, stream);
      break;
    case 1:
      seg_reduce_launch<int32_t>(vals, valid, offsets, n, n_groups, sums, mins,
                                 maxs, counts, tile_groups, partials, stream);
      break;
    case 2:
      seg_reduce_launch<double>(vals, valid, offsets, n, n_groups, sums, mins,
                                maxs, counts, tile_groups, partials, stream);
      break;
    case 3:
      seg_reduce_launch<float>(vals, valid, offsets, n, n_groups, sums, mins,
                               maxs, counts, tile_groups, partials, stream);
      break;
    default:
      fprintf(stderr, "segmented_reduce: bad dtype code %d\n", dtype);
      abort();
  }
}

}  // namespace hsk
