// Long recordings (inference.LongEnhancer; definitions: include/se_hip.h): cut a recording into per-chunk normalised pieces for the
// batched eval forward, and crossfade the enhanced chunks back into one signal.  Both kernels are latency-sized next to the model
// forward: plain loads and stores, no LDS beyond the block reduction, no atomics -- every output element has one writer and the
// sums run in a fixed order, so the results are reproducible.
#include "se_common.h"

constexpr int LG_THREADS = 256;

// One workgroup per chunk.  The source offset starts[k] is arbitrary (in general no multiple of 4 samples): 4-byte loads; the
// destination row is 16-byte aligned (S % 4 == 0, checked by the launcher): 16-byte stores.
__global__ __launch_bounds__(LG_THREADS) void chunk_gather_kernel(const float* __restrict__ x, long long L,
                                                                  const long long* __restrict__ starts, int S,
                                                                  float* __restrict__ chunks, float* __restrict__ c,
                                                                  unsigned char* __restrict__ silent) {
  __shared__ double part[LG_THREADS / 64];
  const int k = blockIdx.x;
  const long long s = starts[k];
  const bool ok = s >= 0 && s <= L - S;
  float* dst = chunks + (size_t)k * S;
  const int S4 = S >> 2;
  double sum = 0.0;
  if (ok) {
    const float* src = x + s;
    for (int q = threadIdx.x; q < S4; q += LG_THREADS) {
      const float4 v = make_float4(src[4 * q], src[4 * q + 1], src[4 * q + 2], src[4 * q + 3]);
      *reinterpret_cast<float4*>(dst + 4 * q) = v;
      sum += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
    }
  } else {                                            // a chunk outside the recording: silence
    for (int q = threadIdx.x; q < S4; q += LG_THREADS) *reinterpret_cast<float4*>(dst + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  sum = wave_sum_d(sum);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < LG_THREADS / 64; ++w) t += part[w];
    const bool quiet = t == 0.0;
    c[k] = quiet ? 1.0f : (float)sqrt((double)S / t);
    silent[k] = quiet ? 1 : 0;
  }
}

extern "C" int se_chunk_gather(const float* x, long long L, const long long* starts, int K, int S, float* chunks, float* c,
                               unsigned char* silent, void* stream) {
  SE_REQUIRE(x && starts && chunks && c && silent, "chunk_gather: null operand");
  SE_REQUIRE(K > 0 && S > 0 && (S & 3) == 0 && L >= S, "chunk_gather: bad sizes (K %d, S %d, L %lld): need S %% 4 == 0 and L >= S", K, S, L);
  SE_REQUIRE((reinterpret_cast<uintptr_t>(chunks) & 15) == 0, "chunk_gather: chunks must be 16-byte aligned");
  hipLaunchKernelGGL(chunk_gather_kernel, dim3(K), dim3(LG_THREADS), 0, as_stream(stream), x, L, starts, S, chunks, c, silent);
  return se_check_launch("se_chunk_gather");
}

// One output sample per lane and trip.  k = the last chunk that starts at or before n (binary search in the ascending starts: K is
// a few thousand for a day of audio, and the table stays in the cache); inside the first V samples of a chunk the previous chunk
// fades out linearly.  A silent chunk contributes 0 through a select, so whatever its row of y holds is never used.
__global__ __launch_bounds__(LG_THREADS) void chunk_assemble_kernel(const float* __restrict__ y, const float* __restrict__ c,
                                                                    const unsigned char* __restrict__ silent,
                                                                    const long long* __restrict__ starts, int K, int S, int V,
                                                                    float* __restrict__ out, long long L) {
  const long long step = (long long)gridDim.x * LG_THREADS;
  for (long long n = (long long)blockIdx.x * LG_THREADS + threadIdx.x; n < L; n += step) {
    int lo = 0, hi = K;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (starts[mid] <= n) lo = mid; else hi = mid;
    }
    const long long i = n - starts[lo];
    float r = 0.f;
    if (i >= 0 && i < S) {                            // always, for starts that begin at 0 and leave no gap
      const float ya = y[(size_t)lo * S + i] / c[lo];
      r = silent[lo] ? 0.f : ya;
      if (lo > 0 && i < V) {
        const long long j = n - starts[lo - 1];
        if (j >= 0 && j < S) {
          const float yb = y[(size_t)(lo - 1) * S + j] / c[lo - 1];
          const float b = silent[lo - 1] ? 0.f : yb;
          const float w = ((float)i + 0.5f) / (float)V;
          r = w * r + (1.0f - w) * b;
        }
      }
    }
    out[n] = r;
  }
}

extern "C" int se_chunk_assemble(const float* y, const float* c, const unsigned char* silent, const long long* starts, int K, int S,
                                 int V, float* out, long long L, void* stream) {
  SE_REQUIRE(y && c && silent && starts && out, "chunk_assemble: null operand");
  SE_REQUIRE(K > 0 && S > 0 && V >= 1 && V <= S && L > 0, "chunk_assemble: bad sizes (K %d, S %d, V %d, L %lld)", K, S, V, L);
  const long long nb = (L + LG_THREADS - 1) / LG_THREADS;
  hipLaunchKernelGGL(chunk_assemble_kernel, dim3((unsigned)(nb > 2048 ? 2048 : nb)), dim3(LG_THREADS), 0, as_stream(stream), y, c,
                     silent, starts, K, S, V, out, L);
  return se_check_launch("se_chunk_assemble");
}
