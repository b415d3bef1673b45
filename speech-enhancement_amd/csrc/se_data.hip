// Dataset kernels: the rational resampler that turns decoded wav files into the resident 16 kHz corpus, and the crop gather that
// cuts one training batch out of it (speech-enhancement_amd/data.py).  Both are HBM-bound and tiny next to a train step; the bar
// is exactness of the definition in include/se_hip.h, no scratch, and every index checked against the arena sizes the caller states.
#include "se_common.h"

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_TILE = 1024;                       // outputs of one workgroup (4 per thread)
constexpr size_t RS_LDS_DEFAULT = 64 * 1024;            // dynamic LDS a kernel gets without raising its limit
constexpr size_t RS_LDS_MAX = 160 * 1024;

// floor division for a possibly negative numerator (b > 0)
static __host__ __device__ __forceinline__ long long fdiv_(long long a, long long b) {
  long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
static __host__ __device__ __forceinline__ long long cdiv_(long long a, long long b) { return -fdiv_(-a, b); }

// input samples a tile of `tile` outputs can touch: i from ceil((j0 down - half) / up) to floor(((j0 + tile - 1) down + half) / up)
static inline long long rs_span(int tile, int up, int down, int ntaps) {
  return ((long long)(tile - 1) * down + (ntaps - 1)) / up + 2;
}
static inline size_t rs_lds_bytes(int tile, int up, int down, int ntaps) {
  return (((size_t)ntaps + 3) & ~(size_t)3) * 4 + (size_t)rs_span(tile, up, down, ntaps) * 4;
}

extern "C" int se_resample_poly_tile(int up, int down, int ntaps) {
  if (up < 1 || down < 1 || ntaps < 1 || (ntaps & 1) == 0) return 0;
  for (int tile = RS_MAX_TILE; tile >= 1; tile >>= 1)
    if (rs_lds_bytes(tile, up, down, ntaps) <= (tile > 1 ? RS_LDS_DEFAULT : RS_LDS_MAX)) return tile;
  return 0;
}

// One workgroup = one tile of one utterance: taps and the input span (zero-extended, so the tap loop has no range test) go to LDS,
// then thread t walks the phase of outputs j0 + t, j0 + t + 256, ...: first tap (j down + half) mod up at input floor((j down + half) / up),
// then taps += up, input -= 1.
template <typename T>
__global__ __launch_bounds__(RS_THREADS) void resample_poly_kernel(const T* __restrict__ x, const long long* __restrict__ utt,
                                                                   const int* __restrict__ tiles, const float* __restrict__ h,
                                                                   float* __restrict__ y, int up, int down, int ntaps, int tile,
                                                                   long long in_total, long long out_total, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* hs = reinterpret_cast<float*>(smem);
  float* xs = hs + ((ntaps + 3) & ~3);
  const int u = tiles[2 * blockIdx.x], j0 = tiles[2 * blockIdx.x + 1];
  const long long in_off = utt[3 * u], n = utt[3 * u + 1], out_off = utt[3 * u + 2];
  const long long n_out = (n * up + down - 1) / down;
  // a table that does not fit the arenas writes nothing (the host checks it too; this keeps a bad table from leaving the buffers)
  if (n < 0 || in_off < 0 || out_off < 0 || in_off + n > in_total || out_off + n_out > out_total || j0 < 0 || j0 >= n_out) return;
  const int half = (ntaps - 1) / 2;
  const long long i_lo = cdiv_((long long)j0 * down - half, up);
  const int span = (int)(((long long)(tile - 1) * down + (ntaps - 1)) / up + 2);
  for (int k = threadIdx.x; k < ntaps; k += RS_THREADS) hs[k] = h[k];
  for (int k = threadIdx.x; k < span; k += RS_THREADS) {
    const long long i = i_lo + k;
    xs[k] = (i >= 0 && i < n) ? (float)x[in_off + i] * scale : 0.f;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < tile; t += RS_THREADS) {
    const long long j = (long long)j0 + t;
    if (j >= n_out) break;
    const long long c = j * down + half;
    int k = (int)(c % up);
    int i = (int)(c / up - i_lo);                       // < span by construction; the loop ends before it goes below 0
    float acc = 0.f;
    for (; k < ntaps; k += up, --i) acc = fmaf(xs[i], hs[k], acc);
    y[out_off + j] = acc;
  }
}

extern "C" int se_resample_poly(const void* x, int x_is_int16, const long long* utt, int n_utt, const int* tiles, int n_tiles,
                                int tile, const float* taps, int ntaps, int up, int down, float* y, long long in_total,
                                long long out_total, void* stream) {
  SE_REQUIRE(x && utt && tiles && taps && y, "resample_poly: null operand");
  SE_REQUIRE(up >= 1 && down >= 1 && ntaps >= 1 && (ntaps & 1) == 1, "resample_poly: bad ratio %d:%d or tap count %d", up, down, ntaps);
  SE_REQUIRE(n_utt > 0 && n_tiles >= 0 && in_total >= 0 && out_total >= 0, "resample_poly: bad table sizes (%d utterances, %d tiles)",
             n_utt, n_tiles);
  SE_REQUIRE(tile >= 1 && tile == se_resample_poly_tile(up, down, ntaps),
             "resample_poly: tile %d is not se_resample_poly_tile(%d, %d, %d) = %d", tile, up, down, ntaps,
             se_resample_poly_tile(up, down, ntaps));
  if (n_tiles == 0) return 0;
  const size_t lds = rs_lds_bytes(tile, up, down, ntaps);
  static unsigned done16 = 0, done32 = 0;
  if (x_is_int16) {
    if (lds > RS_LDS_DEFAULT)
      SE_REQUIRE(se_raise_lds((const void*)resample_poly_kernel<short>, lds, &done16), "resample_poly: cannot raise the LDS limit");
    hipLaunchKernelGGL(resample_poly_kernel<short>, dim3(n_tiles), dim3(RS_THREADS), lds, as_stream(stream),
                       static_cast<const short*>(x), utt, tiles, taps, y, up, down, ntaps, tile, in_total, out_total, 1.0f / 32768.0f);
  } else {
    if (lds > RS_LDS_DEFAULT)
      SE_REQUIRE(se_raise_lds((const void*)resample_poly_kernel<float>, lds, &done32), "resample_poly: cannot raise the LDS limit");
    hipLaunchKernelGGL(resample_poly_kernel<float>, dim3(n_tiles), dim3(RS_THREADS), lds, as_stream(stream),
                       static_cast<const float*>(x), utt, tiles, taps, y, up, down, ntaps, tile, in_total, out_total, 1.0f);
  }
  return se_check_launch("se_resample_poly");
}

// One workgroup per batch row: copies (or tiles) the crop of both signals and reduces the row's statistics in fp64 registers,
// wave shuffles and one LDS step -- a fixed order, so the statistics are reproducible.
constexpr int CG_THREADS = 256;

__global__ __launch_bounds__(CG_THREADS) void crop_gather_kernel(const float* __restrict__ clean_arena,
                                                                 const float* __restrict__ noisy_arena,
                                                                 const long long* __restrict__ rows, int L, long long arena_total,
                                                                 float* __restrict__ clean, float* __restrict__ noisy,
                                                                 float* __restrict__ stats) {
  __shared__ double red[3][CG_THREADS / 64];
  const int b = blockIdx.x;
  const long long off = rows[3 * b], len = rows[3 * b + 1];
  long long start = rows[3 * b + 2];
  const bool tiled = len < L;
  if (tiled) start = 0;
  const bool ok = off >= 0 && len >= 1 && off + len <= arena_total && start >= 0 && (tiled || start + L <= len);
  float* co = clean + (size_t)b * L;
  float* no = noisy + (size_t)b * L;
  double sc = 0.0, sn = 0.0;
  float mx = 0.f;
  if (ok) {
    const float* cs = clean_arena + off + start;
    const float* ns = noisy_arena + off + start;
    for (int t = threadIdx.x; t < L; t += CG_THREADS) {
      const long long i = tiled ? (long long)(t % (int)len) : t;
      const float c = cs[i], v = ns[i];
      co[t] = c;
      no[t] = v;
      sc += (double)c * c;
      sn += (double)v * v;
      mx = fmaxf(mx, fabsf(c));
    }
  } else {                                            // a row outside the arena: silence, which the loader rejects
    for (int t = threadIdx.x; t < L; t += CG_THREADS) co[t] = no[t] = 0.f;
  }
  sc = wave_sum_d(sc);
  sn = wave_sum_d(sn);
  mx = wave_max(mx);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][w] = sc;
    red[1][w] = sn;
    red[2][w] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, c = 0.0, m = 0.0;
    for (int k = 0; k < CG_THREADS / 64; ++k) {
      a += red[0][k];
      c += red[1][k];
      m = fmax(m, red[2][k]);
    }
    stats[3 * b] = (float)a;
    stats[3 * b + 1] = (float)c;
    stats[3 * b + 2] = (float)m;
  }
}

extern "C" int se_crop_gather(const float* clean_arena, const float* noisy_arena, long long arena_total, const long long* rows, int B,
                              int L, float* clean, float* noisy, float* stats, void* stream) {
  SE_REQUIRE(clean_arena && noisy_arena && rows && clean && noisy && stats, "crop_gather: null operand");
  SE_REQUIRE(B > 0 && L > 0 && arena_total > 0, "crop_gather: bad sizes (B %d, L %d, arena %lld)", B, L, arena_total);
  hipLaunchKernelGGL(crop_gather_kernel, dim3(B), dim3(CG_THREADS), 0, as_stream(stream), clean_arena, noisy_arena, rows, L, arena_total,
                     clean, noisy, stats);
  return se_check_launch("se_crop_gather");
}
