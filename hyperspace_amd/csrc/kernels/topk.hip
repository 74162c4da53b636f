// CDNA4 (gfx950 / MI355X) top-k row selection for hyperspace_amd: the rows
// holding the k smallest u64 keys, in ascending row order (ORDER BY ... LIMIT
// without sorting the input).
//
//   threshold  MSD radix select on 8-bit digits.  Per digit that varies, a
//              histogram kernel counts that digit over the valid rows whose
//              higher digits equal the prefix found so far, and a one-block
//              pick kernel scans the 256 bins for the digit that holds the
//              k-th row and advances (prefix, prefix mask, remaining k) in
//              device memory.  The host launches all eight passes up front;
//              a pass over a digit that does not vary returns at once.  A
//              pass reads 8 B/row and writes nothing but 256 counters.
//   emit       stable compaction against the threshold T, in the shape of
//              select_range: a count pass gives every block its (less,
//              equal) pair, one block scans the equal counts into per-block
//              tie allowances and the taken counts into output bases, and
//              the emit pass places rows by ballot rank inside the tile.
//
// Every counter is an integer; the only atomics are integer adds whose sum
// does not depend on arrival order, so the output is identical from run to
// run.  Rows are tiled as in aggregate.hip: TK_TILE rows per tile, blocks
// walk contiguous tile ranges, each lane loads two adjacent keys as one
// 16-byte vector.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace hsk {

namespace {

constexpr int TK_THREADS = 256;
constexpr int TK_WAVES = TK_THREADS / 64;
constexpr int TK_RPT = 8;                      // rows per thread per tile
constexpr int TK_TILE = TK_THREADS * TK_RPT;   // 2048 rows per tile
constexpr int TK_ITERS = TK_RPT / 2;           // 16-byte pair loads per tile
constexpr int TK_MAX_BLOCKS = 2048;            // 256 CUs x 8 blocks/CU
constexpr int TK_BINS = 256;

static_assert(TK_BINS == TK_THREADS, "one thread per histogram bin");

// select state in device memory
constexpr int ST_PREFIX = 0;   // key bits found so far
constexpr int ST_PMASK = 1;    // which bits of ST_PREFIX are final
constexpr int ST_KREM = 2;     // rank of the wanted row inside the prefix

static inline int64_t tk_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct TkGrid {
  int nb;
  int64_t n_tiles;
  int64_t tpb;  // tiles per block
};

static inline TkGrid tk_grid(int64_t n) {
  TkGrid g;
  g.n_tiles = tk_cdiv(n, TK_TILE);
  if (g.n_tiles < 1) g.n_tiles = 1;
  g.tpb = tk_cdiv(g.n_tiles, TK_MAX_BLOCKS);
  g.nb = (int)tk_cdiv(g.n_tiles, g.tpb);
  return g;
}

// Rows r and r + 1 (r even): keys and validity.  A row at or past n comes
// back invalid; the stored key of an invalid row is never looked at.
struct TkPair {
  uint64_t k0, k1;
  uint32_t v0, v1;
};

__device__ __forceinline__ TkPair tk_load_pair(
    const uint64_t* __restrict__ keys, const uint8_t* __restrict__ valid,
    int64_t r, int64_t n) {
  TkPair p;
  p.k0 = 0;
  p.k1 = 0;
  p.v0 = 0;
  p.v1 = 0;
  if (r + 1 < n) {
    ulonglong2 kk = *reinterpret_cast<const ulonglong2*>(keys + r);
    p.k0 = kk.x;
    p.k1 = kk.y;
    uint32_t mm = 0x0101u;
    if (valid != nullptr) mm = *reinterpret_cast<const uint16_t*>(valid + r);
    p.v0 = mm & 0xFFu;
    p.v1 = mm >> 8;
  } else if (r < n) {
    p.k0 = keys[r];
    p.v0 = valid != nullptr ? valid[r] : 1u;
  }
  return p;
}

// One LDS add per distinct digit per wave: lanes find their peers (same
// digit among the participating lanes) with eight ballots and the lowest
// peer adds the group's size.  64 lanes on one digit cost one LDS atomic,
// not 64 serialized ones.  Every lane of the wave must call this.
__device__ __forceinline__ void tk_wave_add(uint32_t* lh, bool part,
                                            uint32_t d, int lane) {
  unsigned long long peers = __ballot(part);
  if (peers == 0ull) return;  // wave-uniform
#pragma unroll
  for (int b = 0; b < 8; b++) {
    bool bit = (d >> b) & 1u;
    unsigned long long m = __ballot(bit);
    peers &= bit ? m : ~m;
  }
  if (part && (__ffsll((long long)peers) - 1) == lane)
    atomicAdd(&lh[d], (uint32_t)__popcll(peers));
}

__global__ void k_tk_init(const uint64_t* __restrict__ keys,
                          const uint64_t* __restrict__ vary, int64_t k,
                          uint64_t* __restrict__ st) {
  // bits that never vary are known from any row
  uint64_t pmask = ~vary[0];
  st[ST_PREFIX] = keys[0] & pmask;
  st[ST_PMASK] = pmask;
  st[ST_KREM] = (uint64_t)k;
}

__global__ __launch_bounds__(TK_THREADS) void k_tk_hist(
    const uint64_t* __restrict__ keys, const uint8_t* __restrict__ valid,
    int64_t n, int shift, const uint64_t* __restrict__ vary,
    const uint64_t* __restrict__ st, unsigned long long* __restrict__ ghist,
    int64_t n_tiles, int64_t tpb) {
  if (((vary[0] >> shift) & 0xFFull) == 0ull) return;  // digit is constant
  __shared__ uint32_t lh[TK_BINS];
  lh[threadIdx.x] = 0;
  __syncthreads();
  uint64_t pmask = st[ST_PMASK];
  uint64_t prefix = st[ST_PREFIX];
  int lane = threadIdx.x & 63;
  int64_t t0 = (int64_t)blockIdx.x * tpb;
  int64_t t1 = t0 + tpb < n_tiles ? t0 + tpb : n_tiles;
  for (int64_t tile = t0; tile < t1; tile++) {
    int64_t ts = tile * TK_TILE;
#pragma unroll
    for (int it = 0; it < TK_ITERS; it++) {
      int64_t r = ts + (int64_t)(it * TK_THREADS + threadIdx.x) * 2;
      TkPair p = tk_load_pair(keys, valid, r, n);
      uint64_t k0 = p.k0, k1 = p.k1;
      bool v0 = p.v0 != 0, v1 = p.v1 != 0;
      bool p0 = v0 && (k0 & pmask) == prefix;
      bool p1 = v1 && (k1 & pmask) == prefix;
      tk_wave_add(lh, p0, (uint32_t)(k0 >> shift) & 0xFFu, lane);
      tk_wave_add(lh, p1, (uint32_t)(k1 >> shift) & 0xFFu, lane);
    }
  }
  __syncthreads();
  uint32_t c = lh[threadIdx.x];
  if (c != 0) atomicAdd(&ghist[threadIdx.x], (unsigned long long)c);
}

// One block: the digit whose bin holds the k_rem-th row (1-based) of the
// current prefix.  When k_rem exceeds the rows there are (k > n_valid) the
// last non-empty bin is taken and k_rem stays above its count, so every
// tie is kept later on.
__global__ __launch_bounds__(TK_BINS) void k_tk_pick(
    int shift, const uint64_t* __restrict__ vary,
    const unsigned long long* __restrict__ ghist, uint64_t* __restrict__ st) {
  if (((vary[0] >> shift) & 0xFFull) == 0ull) return;
  __shared__ unsigned long long incl[TK_BINS];
  int t = threadIdx.x;
  unsigned long long c = ghist[t];
  incl[t] = c;
  __syncthreads();
  for (int off = 1; off < TK_BINS; off <<= 1) {
    unsigned long long v = t >= off ? incl[t - off] : 0ull;
    __syncthreads();
    incl[t] += v;
    __syncthreads();
  }
  unsigned long long total = incl[TK_BINS - 1];
  unsigned long long mine = incl[t];
  unsigned long long before = mine - c;
  unsigned long long k = st[ST_KREM];
  __syncthreads();  // every thread has read k before one of them writes it
  bool hit;
  if (total == 0ull)
    hit = t == 0;  // no valid row at all: any digit, nothing is emitted
  else if (k <= total)
    hit = c != 0ull && before < k && k <= mine;
  else
    hit = c != 0ull && mine == total;
  if (hit) {
    st[ST_PREFIX] |= (uint64_t)t << shift;
    st[ST_PMASK] |= 0xFFull << shift;
    st[ST_KREM] = k - before;
  }
}

__global__ __launch_bounds__(TK_THREADS) void k_tk_count(
    const uint64_t* __restrict__ keys, const uint8_t* __restrict__ valid,
    int64_t n, const uint64_t* __restrict__ st, int64_t* __restrict__ less,
    int64_t* __restrict__ equal, int64_t n_tiles, int64_t tpb) {
  __shared__ uint32_t s_lt[TK_WAVES];
  __shared__ uint32_t s_eq[TK_WAVES];
  uint64_t T = st[ST_PREFIX];
  int lane = threadIdx.x & 63;
  int wave = threadIdx.x >> 6;
  uint32_t lt = 0, eq = 0;
  int64_t t0 = (int64_t)blockIdx.x * tpb;
  int64_t t1 = t0 + tpb < n_tiles ? t0 + tpb : n_tiles;
  for (int64_t tile = t0; tile < t1; tile++) {
    int64_t ts = tile * TK_TILE;
#pragma unroll
    for (int it = 0; it < TK_ITERS; it++) {
      int64_t r = ts + (int64_t)(it * TK_THREADS + threadIdx.x) * 2;
      TkPair p = tk_load_pair(keys, valid, r, n);
      uint64_t k0 = p.k0, k1 = p.k1;
      bool v0 = p.v0 != 0, v1 = p.v1 != 0;
      lt += (uint32_t)(v0 && k0 < T) + (uint32_t)(v1 && k1 < T);
      eq += (uint32_t)(v0 && k0 == T) + (uint32_t)(v1 && k1 == T);
    }
  }
  for (int d = 32; d > 0; d >>= 1) {
    lt += __shfl_down(lt, d);
    eq += __shfl_down(eq, d);
  }
  if (lane == 0) {
    s_lt[wave] = lt;
    s_eq[wave] = eq;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t a = 0, b = 0;
    for (int w = 0; w < TK_WAVES; w++) {
      a += s_lt[w];
      b += s_eq[w];
    }
    less[blockIdx.x] = a;
    equal[blockIdx.x] = b;
  }
}

constexpr int TK_SCAN_CHUNK = TK_MAX_BLOCKS / TK_THREADS;  // 8 blocks/thread

__device__ __forceinline__ int64_t tk_block_scan(int64_t* s, int t,
                                                 int64_t v) {
  // exclusive prefix of v over the block's threads; s[TK_THREADS - 1]
  // holds the total afterwards
  s[t] = v;
  __syncthreads();
  for (int off = 1; off < TK_THREADS; off <<= 1) {
    int64_t u = t >= off ? s[t - off] : 0;
    __syncthreads();
    s[t] += u;
    __syncthreads();
  }
  return s[t] - v;
}

// One block.  Ties first: block b may keep allow[b] = clamp(quota - ties
// before b, 0, equal[b]) of its tie rows, the first ones in row order.
// Then base[b] = rows taken before block b, and the total.
__global__ __launch_bounds__(TK_THREADS) void k_tk_scan(
    const int64_t* __restrict__ less, const int64_t* __restrict__ equal,
    int nb, const uint64_t* __restrict__ st, bool keep_ties,
    int64_t* __restrict__ allow, int64_t* __restrict__ base,
    int64_t* __restrict__ total) {
  __shared__ int64_t s[TK_THREADS];
  int t = threadIdx.x;
  int start = t * TK_SCAN_CHUNK;
  int end = start + TK_SCAN_CHUNK < nb ? start + TK_SCAN_CHUNK : nb;
  int64_t quota = keep_ties ? INT64_MAX : (int64_t)st[ST_KREM];
  int64_t e = 0;
  for (int i = start; i < end; i++) e += equal[i];
  int64_t ebase = tk_block_scan(s, t, e);
  __syncthreads();
  int64_t taken = 0;
  int64_t tk[TK_SCAN_CHUNK];
#pragma unroll
  for (int j = 0; j < TK_SCAN_CHUNK; j++) {
    int i = start + j;
    tk[j] = 0;
    if (i < end) {
      int64_t eq = equal[i];
      int64_t room = quota - ebase;
      int64_t a = room <= 0 ? 0 : (room < eq ? room : eq);
      allow[i] = a;
      ebase += eq;
      tk[j] = less[i] + a;
      taken += tk[j];
    }
  }
  int64_t obase = tk_block_scan(s, t, taken);
  if (t == TK_THREADS - 1) total[0] = s[t];
#pragma unroll
  for (int j = 0; j < TK_SCAN_CHUNK; j++) {
    int i = start + j;
    if (i < end) {
      base[i] = obase;
      obase += tk[j];
    }
  }
}

__global__ __launch_bounds__(TK_THREADS) void k_tk_emit(
    const uint64_t* __restrict__ keys, const uint8_t* __restrict__ valid,
    int64_t n, const uint64_t* __restrict__ st,
    const int64_t* __restrict__ less, const int64_t* __restrict__ allow,
    const int64_t* __restrict__ base, int64_t* __restrict__ out,
    int64_t n_out, int64_t n_tiles, int64_t tpb) {
  __shared__ uint32_t s_lt[TK_ITERS][TK_WAVES];
  __shared__ uint32_t s_eq[TK_ITERS][TK_WAVES];
  int64_t allow_b = allow[blockIdx.x];
  int64_t want = less[blockIdx.x] + allow_b;
  if (want == 0) return;  // block-uniform
  uint64_t T = st[ST_PREFIX];
  int lane = threadIdx.x & 63;
  int wave = threadIdx.x >> 6;
  unsigned long long below = (1ull << lane) - 1ull;
  int64_t o = base[blockIdx.x];  // next output slot of the block
  int64_t eq_run = 0;            // tie rows of the block seen so far
  int64_t done = 0;              // rows of the block placed so far
  int64_t t0 = (int64_t)blockIdx.x * tpb;
  int64_t t1 = t0 + tpb < n_tiles ? t0 + tpb : n_tiles;
  // every thread derives the same running totals from LDS, so the loop
  // exit is block-uniform
  for (int64_t tile = t0; tile < t1 && done < want; tile++) {
    int64_t ts = tile * TK_TILE;
#pragma unroll
    for (int it = 0; it < TK_ITERS; it++) {
      int64_t r = ts + (int64_t)(it * TK_THREADS + threadIdx.x) * 2;
      TkPair p = tk_load_pair(keys, valid, r, n);
      uint64_t k0 = p.k0, k1 = p.k1;
      bool v0 = p.v0 != 0, v1 = p.v1 != 0;
      bool l0 = v0 && k0 < T, l1 = v1 && k1 < T;
      bool e0 = v0 && k0 == T, e1 = v1 && k1 == T;
      unsigned long long be0 = __ballot(e0), be1 = __ballot(e1);
      unsigned long long bl0 = __ballot(l0), bl1 = __ballot(l1);
      if (lane == 0) {
        s_lt[it][wave] = (uint32_t)(__popcll(bl0) + __popcll(bl1));
        s_eq[it][wave] = (uint32_t)(__popcll(be0) + __popcll(be1));
      }
      __syncthreads();
      // the LDS slots of this iteration are next written a tile later,
      // behind the barriers of the other iterations
      int64_t e_before = eq_run;  // ties ahead of this wave
      int64_t o_before = 0;       // rows taken by earlier waves
      int64_t e_all = eq_run, o_all = 0;
#pragma unroll
      for (int w = 0; w < TK_WAVES; w++) {
        int64_t we = s_eq[it][w];
        int64_t room = allow_b - e_all;
        int64_t wt = s_lt[it][w] + (room <= 0 ? 0 : (room < we ? room : we));
        if (w < wave) {
          e_before += we;
          o_before += wt;
        }
        e_all += we;
        o_all += wt;
      }
      int64_t rank_e =
          e_before + __popcll(be0 & below) + __popcll(be1 & below);
      bool t0b = l0 || (e0 && rank_e < allow_b);
      bool t1b = l1 || (e1 && rank_e + (int64_t)e0 < allow_b);
      unsigned long long bt0 = __ballot(t0b), bt1 = __ballot(t1b);
      int64_t pos =
          o + o_before + __popcll(bt0 & below) + __popcll(bt1 & below);
      if (t0b) {
        if (pos < n_out) out[pos] = r;
        pos++;
      }
      if (t1b && pos < n_out) out[pos] = r + 1;
      o += o_all;
      done += o_all;
      eq_run = e_all;
    }
  }
}

}  // namespace

int64_t topk_tile_size() { return TK_TILE; }

int64_t topk_num_blocks(int64_t n) { return tk_grid(n).nb; }

int64_t topk_scratch_size(int64_t n) {
  return 8 * TK_BINS + 8 + 4 * (int64_t)tk_grid(n).nb;
}

namespace {

struct TkScratch {
  unsigned long long* ghist;  // 8 passes x 256 bins
  uint64_t* vary;
  uint64_t* st;
  int64_t* total;
  int64_t *less, *equal, *allow, *base;
};

static TkScratch tk_scratch(int64_t* scratch, int nb) {
  TkScratch s;
  s.ghist = (unsigned long long*)scratch;
  s.vary = (uint64_t*)(scratch + 8 * TK_BINS);
  s.st = s.vary + 1;
  s.total = scratch + 8 * TK_BINS + 7;
  s.less = scratch + 8 * TK_BINS + 8;
  s.equal = s.less + nb;
  s.allow = s.equal + nb;
  s.base = s.allow + nb;
  return s;
}

}  // namespace

int64_t* topk_select(const uint64_t* keys, const uint8_t* valid, int64_t n,
                     int64_t k, bool keep_ties, int64_t* scratch,
                     hipStream_t stream) {
  TkGrid g = tk_grid(n);
  TkScratch s = tk_scratch(scratch, g.nb);
  key_varying_bits(keys, n, s.vary, stream);
  hipLaunchKernelGGL(k_tk_init, dim3(1), dim3(1), 0, stream, keys, s.vary, k,
                     s.st);
  for (int pass = 0; pass < 8; pass++) {
    int shift = 56 - 8 * pass;
    unsigned long long* h = s.ghist + pass * TK_BINS;
    hipLaunchKernelGGL(k_tk_hist, dim3(g.nb), dim3(TK_THREADS), 0, stream,
                       keys, valid, n, shift, s.vary, s.st, h, g.n_tiles,
                       g.tpb);
    hipLaunchKernelGGL(k_tk_pick, dim3(1), dim3(TK_BINS), 0, stream, shift,
                       s.vary, h, s.st);
  }
  hipLaunchKernelGGL(k_tk_count, dim3(g.nb), dim3(TK_THREADS), 0, stream,
                     keys, valid, n, s.st, s.less, s.equal, g.n_tiles, g.tpb);
  hipLaunchKernelGGL(k_tk_scan, dim3(1), dim3(TK_THREADS), 0, stream, s.less,
                     s.equal, g.nb, s.st, keep_ties, s.allow, s.base,
                     s.total);
  return s.total;
}

void topk_emit(const uint64_t* keys, const uint8_t* valid, int64_t n,
               const int64_t* scratch, int64_t* out, int64_t n_out,
               hipStream_t stream) {
  if (n_out == 0) return;
  TkGrid g = tk_grid(n);
  TkScratch s = tk_scratch(const_cast<int64_t*>(scratch), g.nb);
  hipLaunchKernelGGL(k_tk_emit, dim3(g.nb), dim3(TK_THREADS), 0, stream, keys,
                     valid, n, s.st, s.less, s.allow, s.base, out, n_out,
                     g.n_tiles, g.tpb);
}

}  // namespace hsk
