// Streaming enhancement (inference.StreamEnhancer; definitions: include/se_hip.h): the state of B live streams -- a ring of the
// last W input samples, a sample counter and the withheld tail of the previous estimate per row -- stays on the device and is
// advanced by two kernels around the batched eval forward, so that one step is window -> STFT -> generator -> iSTFT -> emit without
// a host synchronisation (one HIP graph).  Both kernels are latency-sized next to the forward, like se_long.hip: plain loads and
// stores, no LDS beyond the block reduction, no atomics -- every element has one writer and the sums run in a fixed order.
#include "se_common.h"

constexpr int ST_THREADS = 256;

// One workgroup per row.  The counter is a multiple of H in normal use, so with H % 4 == 0 and W % 4 == 0 every quad of the ring is
// 16-byte aligned and does not straddle the ring's end; a counter that is no multiple of 4 (only a caller that wrote pos itself can
// produce one) takes 4-byte accesses with a wrap per element.  The H slots the block overwrites hold samples [n - W - H, n - W): the
// window reads [n - W, n - H) from the ring and [n - H, n) from the block, so no slot is read after it was written.
__global__ __launch_bounds__(ST_THREADS) void stream_window_kernel(const float* __restrict__ block, float* ring,
                                                                   const long long* __restrict__ pos, int H, int W,
                                                                   float* __restrict__ window, float* __restrict__ c,
                                                                   unsigned char* __restrict__ silent) {
  __shared__ double part[ST_THREADS / 64];
  const int b = blockIdx.x;
  const long long p = pos[b];
  const float* src = block + (size_t)b * H;
  float* rg = ring + (size_t)b * W;
  float* dst = window + (size_t)b * W;
  const int W4 = W >> 2, H4 = H >> 2, old = W - H;     // old: window samples that come from the ring
  double sum = 0.0;
  if (p < 0) {                                         // not a state this code produces: the ring is left alone, the window is silence
    for (int q = threadIdx.x; q < W4; q += ST_THREADS) *reinterpret_cast<float4*>(dst + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    const int p0 = (int)(p % W);                       // slot of the block's first sample
    const bool quads = (p & 3) == 0;
    const long long n = p + H;
    const int fill = n >= W ? 0 : (int)(W - n);        // window[i] = 0 for i < fill: sample n - W + i does not exist yet
    for (int q = threadIdx.x; q < H4; q += ST_THREADS) {
      const float4 v = *reinterpret_cast<const float4*>(src + 4 * q);
      int s = p0 + 4 * q;
      if (s >= W) s -= W;
      if (quads) {
        *reinterpret_cast<float4*>(rg + s) = v;
      } else {
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int t = 0; t < 4; ++t) rg[s + t >= W ? s + t - W : s + t] = e[t];
      }
    }
    for (int q = threadIdx.x; q < W4; q += ST_THREADS) {
      const int i = 4 * q;
      float4 v;
      if (i >= old) {
        v = *reinterpret_cast<const float4*>(src + (i - old));
      } else {
        int s = p0 + H + i;                            // (n - W + i) mod W, p0 + H + i < 3 W
        if (s >= W) s -= W;
        if (s >= W) s -= W;
        if (quads) {                                   // fill is a multiple of 4 as well: a quad is all history or all zeros
          v = i < fill ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(rg + s);
        } else {
          float e[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) e[t] = i + t < fill ? 0.f : rg[s + t >= W ? s + t - W : s + t];
          v = make_float4(e[0], e[1], e[2], e[3]);
        }
      }
      *reinterpret_cast<float4*>(dst + i) = v;
      sum += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
    }
  }
  sum = wave_sum_d(sum);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < ST_THREADS / 64; ++w) t += part[w];
    const bool quiet = t == 0.0;
    const long long n = p + H;
    const double r = (double)(n < W ? n : (long long)W);
    c[b] = quiet ? 1.0f : (float)sqrt(r / t);
    silent[b] = quiet ? 1 : 0;
  }
}

extern "C" int se_stream_window(const float* block, float* ring, const long long* pos, int B, int H, int W, float* window, float* c,
                                unsigned char* silent, void* stream) {
  SE_REQUIRE(block && ring && pos && window && c && silent, "stream_window: null operand");
  SE_REQUIRE(B > 0 && H > 0 && (H & 3) == 0 && W > 0 && (W & 3) == 0 && H <= W,
             "stream_window: bad sizes (B %d, H %d, W %d): need H %% 4 == 0, W %% 4 == 0 and H <= W", B, H, W);
  SE_REQUIRE(((reinterpret_cast<uintptr_t>(block) | reinterpret_cast<uintptr_t>(ring) | reinterpret_cast<uintptr_t>(window)) & 15) == 0,
             "stream_window: block, ring and window must be 16-byte aligned");
  SE_REQUIRE((reinterpret_cast<uintptr_t>(pos) & 7) == 0, "stream_window: pos must be 8-byte aligned");
  hipLaunchKernelGGL(stream_window_kernel, dim3(B), dim3(ST_THREADS), 0, as_stream(stream), block, ring, pos, H, W, window, c, silent);
  return se_check_launch("se_stream_window");
}

// One workgroup per row, lane j of a trip owns out[j] and tail[j]: it reads tail[j] for the fade before it overwrites it, so both
// have one writer and no ordering between lanes is needed.  The counter is read by every lane before the barrier and advanced by
// lane 0 after it.  A silent row contributes 0 through a select, so whatever its row of y holds is never used.
__global__ __launch_bounds__(ST_THREADS) void stream_emit_kernel(const float* __restrict__ y, const float* __restrict__ c,
                                                                 const unsigned char* __restrict__ silent, float* __restrict__ tail,
                                                                 long long* pos, int H, int W, int D, int V,
                                                                 float* __restrict__ out) {
  const int b = blockIdx.x;
  const long long p = pos[b];
  const float cb = c[b];
  const bool quiet = silent[b] != 0;
  const float* yr = y + (size_t)b * W;
  float* tl = tail + (size_t)b * D;
  float* o = out + (size_t)b * H;
  const int top = H > D ? H : D;
  for (int j = threadIdx.x; j < top; j += ST_THREADS) {
    if (j < H) {
      const float ya = yr[W - H - D + j] / cb;
      float v = quiet ? 0.f : ya;
      if (j < V) {
        const float w = ((float)j + 0.5f) / (float)V;
        v = w * v + (1.0f - w) * tl[j];
      }
      o[j] = p - D + j < 0 ? 0.f : v;                  // global sample n - H - D + j with n = p + H
    }
    if (j < D) {
      const float yt = yr[W - D + j] / cb;
      tl[j] = quiet ? 0.f : yt;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) pos[b] = p + H;
}

extern "C" int se_stream_emit(const float* y, const float* c, const unsigned char* silent, float* tail, long long* pos, int B, int H,
                              int W, int A, int V, float* out, void* stream) {
  SE_REQUIRE(y && c && silent && pos && out, "stream_emit: null operand");
  SE_REQUIRE(B > 0 && H > 0 && (H & 3) == 0 && W > 0 && A >= 0 && V >= 1 && V <= H && (long long)H + A + V <= W,
             "stream_emit: bad sizes (B %d, H %d, W %d, A %d, V %d): need H %% 4 == 0, 1 <= V <= H, A >= 0 and H + A + V <= W", B, H, W, A, V);
  SE_REQUIRE(tail, "stream_emit: null tail (D = A + V >= 1 floats per row)");
  SE_REQUIRE((reinterpret_cast<uintptr_t>(pos) & 7) == 0, "stream_emit: pos must be 8-byte aligned");
  hipLaunchKernelGGL(stream_emit_kernel, dim3(B), dim3(ST_THREADS), 0, as_stream(stream), y, c, silent, tail, pos, H, W, A + V, V, out);
  return se_check_launch("se_stream_emit");
}
