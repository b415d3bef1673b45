// Reverse-diffusion sampler of the TSC hybrid without the host (speech-enhancement_amd/sampler.py): the step index, the utterance
// counter and the seed live in device memory, so one captured reverse step can be replayed for every step of every utterance.
//   se_sampler_begin    audio = noisy = wrap_pad(x) * c
//   se_sampler_update   the [B, L] update of one reverse step, the Gaussian noise drawn in the kernel (Philox4x32-10 + Box-Muller)
//   se_sampler_advance  n -> n - 1 (wrapping to steps - 1 and counting the utterance), d = row n of the step-embedding table
//   se_philox_normal    the generator alone (tests)
// and the forward process of its training step with the same generator (speech-enhancement_amd/tsc_diffusion.py):
//   se_diffuse_draw_steps  one diffusion step per clip
//   se_diffuse_noise       clip scaling + add_noise of a [B, L] batch in one launch, the noise supplied or drawn in the kernel
// All of them are HBM-bound and tiny next to the generator they sit behind; the bar is the definition in include/se_hip.h, no scratch,
// and a draw that depends on (seed, run, n, element) only.
#include "se_common.h"
#include <stdint.h>

constexpr int SP_THREADS = 256;
constexpr int SP_EMB = 64;                               // width of the projected step embedding (MergeBlock: 64 channels)

struct u32x4_ {
  uint32_t x, y, z, w;
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
static __device__ __forceinline__ u32x4_ philox4x32_10_(u32x4_ c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
    u32x4_ o;
    o.x = (uint32_t)(p1 >> 32) ^ c.y ^ k0;
    o.y = (uint32_t)p1;
    o.z = (uint32_t)(p0 >> 32) ^ c.w ^ k1;
    o.w = (uint32_t)p0;
    c = o;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// one Box-Muller pair of two words: u = (w + 0.5) 2^-32 is in (0, 1], never 0
static __device__ __forceinline__ void box_muller_(uint32_t wa, uint32_t wb, float& z0, float& z1) {
  const float ua = ((float)wa + 0.5f) * 2.3283064365386963e-10f;
  const float ub = ((float)wb + 0.5f) * 2.3283064365386963e-10f;
  const float r = sqrtf(-2.0f * logf(ua));
  const float t = 6.283185307179586f * ub;
  z0 = r * cosf(t);
  z1 = r * sinf(t);
}

static __device__ __forceinline__ float4 normals4_(u32x4_ w) {
  float4 z;
  box_muller_(w.x, w.y, z.x, z.y);
  box_muller_(w.z, w.w, z.z, z.w);
  return z;
}

__global__ __launch_bounds__(SP_THREADS) void philox_normal_kernel(uint32_t k0, uint32_t k1, uint32_t c2, uint32_t c3,
                                                                   uint64_t first_group, long long n_groups,
                                                                   uint32_t* __restrict__ words, float* __restrict__ normals) {
  const long long i = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i >= n_groups) return;
  const uint64_t g = first_group + (uint64_t)i;
  const u32x4_ w = philox4x32_10_({(uint32_t)g, (uint32_t)(g >> 32), c2, c3}, k0, k1);
  if (words) {
    uint32_t* o = words + 4 * i;
    o[0] = w.x, o[1] = w.y, o[2] = w.z, o[3] = w.w;
  }
  if (normals) {
    const float4 z = normals4_(w);
    float* o = normals + 4 * i;
    o[0] = z.x, o[1] = z.y, o[2] = z.z, o[3] = z.w;
  }
}

extern "C" int se_philox_normal(unsigned long long seed, unsigned c2, unsigned c3, unsigned long long first_group, long long n_groups,
                                unsigned* out_words, float* out_normals, void* stream) {
  SE_REQUIRE(out_words || out_normals, "philox_normal: no output");
  SE_REQUIRE(n_groups >= 0 && n_groups <= ((long long)1 << 40), "philox_normal: bad group count %lld", n_groups);
  if (n_groups == 0) return 0;
  hipLaunchKernelGGL(philox_normal_kernel, dim3((unsigned)((n_groups + SP_THREADS - 1) / SP_THREADS)), dim3(SP_THREADS), 0,
                     as_stream(stream), (uint32_t)seed, (uint32_t)(seed >> 32), c2, c3, (uint64_t)first_group, n_groups, out_words,
                     out_normals);
  return se_check_launch("se_philox_normal");
}

// One thread = one group of four flat elements 4g .. 4g + 3 of the [B, L] tensors (rows are contiguous, so the flat index ignores
// them; only the de-normalisation looks up its row).  VEC: audio / noisy / eps are 16-byte aligned, so every full group is one
// 16-byte access whatever L is; the last group of a tensor whose size is no multiple of 4, and every group of an unaligned tensor,
// goes element by element.  The supplied-noise slice of step k starts at k B L floats: aligned only where B L is a multiple of 4,
// tested on its own.
template <bool VEC>
__global__ __launch_bounds__(SP_THREADS) void sampler_update_kernel(float* __restrict__ audio, const float* __restrict__ noisy,
                                                                    const float* __restrict__ eps, const float* __restrict__ coef,
                                                                    const int* __restrict__ n_ptr, int steps,
                                                                    const float* __restrict__ noise,
                                                                    const unsigned long long* __restrict__ seed_ptr,
                                                                    const unsigned* __restrict__ run_ptr,
                                                                    const float* __restrict__ c_inv, float gamma, int clamp,
                                                                    long long L, long long total) {
  const int n = *n_ptr;                                   // read only: other workgroups of this launch are still reading it
  if (n < 0 || n >= steps) return;                        // a step outside the table writes nothing
  const long long g = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
  const long long i0 = 4 * g;
  if (i0 >= total) return;
  const int cnt = (int)(total - i0 < 4 ? total - i0 : 4);
  const float c1 = coef[4 * n], c2 = coef[4 * n + 1], c3 = coef[4 * n + 2], sigma = coef[4 * n + 3];
  float a[4], y[4], e[4], z[4] = {0.f, 0.f, 0.f, 0.f};
  const bool full = VEC && cnt == 4;
  if (full) {
    const float4 va = *reinterpret_cast<const float4*>(audio + i0), vy = *reinterpret_cast<const float4*>(noisy + i0),
                 ve = *reinterpret_cast<const float4*>(eps + i0);
    a[0] = va.x, a[1] = va.y, a[2] = va.z, a[3] = va.w;
    y[0] = vy.x, y[1] = vy.y, y[2] = vy.z, y[3] = vy.w;
    e[0] = ve.x, e[1] = ve.y, e[2] = ve.z, e[3] = ve.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool ok = j < cnt;
      a[j] = ok ? audio[i0 + j] : 0.f;
      y[j] = ok ? noisy[i0 + j] : 0.f;
      e[j] = ok ? eps[i0 + j] : 0.f;
    }
  }
  float o[4];
  if (n > 0) {
    if (noise) {
      const float* nz = noise + (long long)(steps - 1 - n) * total + i0;
      if (cnt == 4 && (reinterpret_cast<uintptr_t>(nz) & 15) == 0) {
        const float4 vz = *reinterpret_cast<const float4*>(nz);
        z[0] = vz.x, z[1] = vz.y, z[2] = vz.z, z[3] = vz.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = j < cnt ? nz[j] : 0.f;
      }
    } else {
      const unsigned long long seed = *seed_ptr;
      const float4 vz = normals4_(philox4x32_10_({(uint32_t)g, (uint32_t)((uint64_t)g >> 32), (uint32_t)n, *run_ptr},
                                                 (uint32_t)seed, (uint32_t)(seed >> 32)));
      z[0] = vz.x, z[1] = vz.y, z[2] = vz.z, z[3] = vz.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = fmaf(sigma, z[j], fmaf(-c3, e[j], fmaf(c2, y[j], c1 * a[j])));
  } else {
    const float omg = 1.0f - gamma;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = fmaf(omg, fmaf(c1, a[j], -(c3 * e[j])), gamma * y[j]);
      if (clamp) v = fminf(fmaxf(v, -1.0f), 1.0f);
      if (c_inv && j < cnt) v *= 1.0f / c_inv[(i0 + j) / L];
      o[j] = v;
    }
  }
  if (full) {
    *reinterpret_cast<float4*>(audio + i0) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) audio[i0 + j] = o[j];
  }
}

extern "C" int se_sampler_update(float* audio, const float* noisy, const float* eps, const float* coef, const int* n, int steps,
                                 const float* noise, const unsigned long long* seed, const unsigned* run, const float* c_inv,
                                 float gamma, int clamp, int B, long long L, void* stream) {
  SE_REQUIRE(audio && noisy && eps && coef && n, "sampler_update: null operand");
  SE_REQUIRE(noise || (seed && run), "sampler_update: neither a noise buffer nor a seed and a run counter");
  SE_REQUIRE(B > 0 && L > 0 && steps > 0, "sampler_update: bad sizes (B %d, L %lld, steps %d)", B, L, steps);
  const long long total = (long long)B * L, groups = (total + 3) / 4;
  SE_REQUIRE(groups <= ((long long)1 << 38), "sampler_update: %lld elements are more than one launch covers", total);
  const dim3 grid((unsigned)((groups + SP_THREADS - 1) / SP_THREADS));
  const bool vec = ((reinterpret_cast<uintptr_t>(audio) | reinterpret_cast<uintptr_t>(noisy) | reinterpret_cast<uintptr_t>(eps)) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(sampler_update_kernel<true>, grid, dim3(SP_THREADS), 0, as_stream(stream), audio, noisy, eps, coef, n, steps,
                       noise, seed, run, c_inv, gamma, clamp, L, total);
  else
    hipLaunchKernelGGL(sampler_update_kernel<false>, grid, dim3(SP_THREADS), 0, as_stream(stream), audio, noisy, eps, coef, n, steps,
                       noise, seed, run, c_inv, gamma, clamp, L, total);
  return se_check_launch("se_sampler_update");
}

// ---- forward process of the hybrid's training step (speech-enhancement_amd/tsc_diffusion.py; core/function.py:25-44, 647-659) ----
// One Philox call per row: word 0 of counter (b, 0, c2, c3) scaled to [0, steps) in exact integer arithmetic.
__global__ __launch_bounds__(SP_THREADS) void diffuse_draw_steps_kernel(uint32_t k0, uint32_t k1, uint32_t c2, uint32_t c3, int B,
                                                                        uint32_t steps, long long* __restrict__ t_out) {
  const int b = blockIdx.x * SP_THREADS + threadIdx.x;
  if (b >= B) return;
  const u32x4_ w = philox4x32_10_({(uint32_t)b, 0u, c2, c3}, k0, k1);
  t_out[b] = (long long)(((uint64_t)w.x * steps) >> 32);
}

extern "C" int se_diffuse_draw_steps(unsigned long long seed, unsigned c2, unsigned c3, int B, int steps, long long* t_out,
                                     void* stream) {
  SE_REQUIRE(t_out, "diffuse_draw_steps: null output");
  SE_REQUIRE(B > 0 && steps > 0, "diffuse_draw_steps: bad sizes (B %d, steps %d)", B, steps);
  hipLaunchKernelGGL(diffuse_draw_steps_kernel, dim3((unsigned)((B + SP_THREADS - 1) / SP_THREADS)), dim3(SP_THREADS), 0,
                     as_stream(stream), (uint32_t)seed, (uint32_t)(seed >> 32), c2, c3, B, (uint32_t)steps, t_out);
  return se_check_launch("se_diffuse_draw_steps");
}

// the five coefficients of a row's diffusion step and its clip scale; a step outside the table selects zeros for the whole row
struct diffuse_row_ {
  float cb, A, Bn, S, G, H;
  bool ok;
};

static __device__ __forceinline__ diffuse_row_ diffuse_row_load_(const float* __restrict__ c, const float* __restrict__ coef,
                                                                  const long long* __restrict__ t, int steps, long long b) {
  diffuse_row_ r = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, false};
  const long long k = t[b];
  if (k >= 0 && k < steps) {                              // checked before the table is indexed
    const float* q = coef + 5 * k;
    r.cb = c[b], r.A = q[0], r.Bn = q[1], r.S = q[2], r.G = q[3], r.H = q[4];
    r.ok = true;
  }
  return r;
}

// One thread = one group of four flat elements 4g .. 4g + 3 of the [B, L] tensors, as in sampler_update_kernel: the Philox group is
// the flat group, so a draw does not depend on L or on the launch, and a group may straddle rows (the row's values are reloaded where
// the row changes: L may be 1).  VEC: all operands are 16-byte aligned, so every full group is one 16-byte access per tensor.
template <bool VEC>
__global__ __launch_bounds__(SP_THREADS) void diffuse_noise_kernel(const float* __restrict__ clean, const float* __restrict__ noisy,
                                                                   const float* __restrict__ c, const float* __restrict__ coef,
                                                                   const long long* __restrict__ t, int steps,
                                                                   const float* __restrict__ noise, uint32_t k0, uint32_t k1,
                                                                   uint32_t c2, uint32_t c3, long long L, long long total,
                                                                   float* __restrict__ noisy_n, float* __restrict__ x_t,
                                                                   float* __restrict__ combine) {
  const long long g = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
  const long long i0 = 4 * g;
  if (i0 >= total) return;
  const int cnt = (int)(total - i0 < 4 ? total - i0 : 4);
  const bool full = VEC && cnt == 4;
  float a[4], y[4], z[4];
  if (full) {
    const float4 va = *reinterpret_cast<const float4*>(clean + i0), vy = *reinterpret_cast<const float4*>(noisy + i0);
    a[0] = va.x, a[1] = va.y, a[2] = va.z, a[3] = va.w;
    y[0] = vy.x, y[1] = vy.y, y[2] = vy.z, y[3] = vy.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool ok = j < cnt;
      a[j] = ok ? clean[i0 + j] : 0.f;
      y[j] = ok ? noisy[i0 + j] : 0.f;
    }
  }
  if (noise) {
    if (full) {
      const float4 vz = *reinterpret_cast<const float4*>(noise + i0);
      z[0] = vz.x, z[1] = vz.y, z[2] = vz.z, z[3] = vz.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) z[j] = j < cnt ? noise[i0 + j] : 0.f;
    }
  } else {
    const float4 vz = normals4_(philox4x32_10_({(uint32_t)g, (uint32_t)((uint64_t)g >> 32), c2, c3}, k0, k1));
    z[0] = vz.x, z[1] = vz.y, z[2] = vz.z, z[3] = vz.w;
  }
  long long b = i0 / L, r = i0 - b * L;                   // row and column of element i0; i0 < total, so b < B
  diffuse_row_ w = diffuse_row_load_(c, coef, t, steps, b);
  float on[4], ox[4], oc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // xc, xn: one rounded product each (not contracted into the sums that use them), so noisy_n is torch's noisy * c bit for bit
    const float xc = __fmul_rn(w.cb, a[j]), xn = __fmul_rn(w.cb, y[j]);
    on[j] = w.ok ? xn : 0.f;
    ox[j] = w.ok ? fmaf(w.S, z[j], fmaf(w.Bn, xn, w.A * xc)) : 0.f;
    oc[j] = w.ok ? fmaf(w.H, z[j], w.G * __fsub_rn(xn, xc)) : 0.f;
    if (++r == L && j + 1 < cnt) {                        // the next element opens row b + 1 (< B: it is below total)
      r = 0;
      w = diffuse_row_load_(c, coef, t, steps, ++b);
    }
  }
  if (full) {
    *reinterpret_cast<float4*>(noisy_n + i0) = make_float4(on[0], on[1], on[2], on[3]);
    *reinterpret_cast<float4*>(x_t + i0) = make_float4(ox[0], ox[1], ox[2], ox[3]);
    *reinterpret_cast<float4*>(combine + i0) = make_float4(oc[0], oc[1], oc[2], oc[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) noisy_n[i0 + j] = on[j], x_t[i0 + j] = ox[j], combine[i0 + j] = oc[j];
  }
}

extern "C" int se_diffuse_noise(const float* clean, const float* noisy, const float* c, const float* coef, const long long* t,
                                const float* noise, unsigned long long seed, unsigned c2, unsigned c3, int B, long long L, int steps,
                                float* noisy_n, float* x_t, float* combine, void* stream) {
  SE_REQUIRE(clean && noisy && c && coef && t && noisy_n && x_t && combine, "diffuse_noise: null operand");
  SE_REQUIRE(B > 0 && L > 0 && steps > 0, "diffuse_noise: bad sizes (B %d, L %lld, steps %d)", B, L, steps);
  SE_REQUIRE(L <= ((long long)1 << 40) / B, "diffuse_noise: %d x %lld elements are more than one launch covers", B, L);
  const long long total = (long long)B * L, groups = (total + 3) / 4;
  const dim3 grid((unsigned)((groups + SP_THREADS - 1) / SP_THREADS));
  const uintptr_t bits = reinterpret_cast<uintptr_t>(clean) | reinterpret_cast<uintptr_t>(noisy) | reinterpret_cast<uintptr_t>(noise) |
                         reinterpret_cast<uintptr_t>(noisy_n) | reinterpret_cast<uintptr_t>(x_t) | reinterpret_cast<uintptr_t>(combine);
  if ((bits & 15) == 0)
    hipLaunchKernelGGL(diffuse_noise_kernel<true>, grid, dim3(SP_THREADS), 0, as_stream(stream), clean, noisy, c, coef, t, steps, noise,
                       (uint32_t)seed, (uint32_t)(seed >> 32), c2, c3, L, total, noisy_n, x_t, combine);
  else
    hipLaunchKernelGGL(diffuse_noise_kernel<false>, grid, dim3(SP_THREADS), 0, as_stream(stream), clean, noisy, c, coef, t, steps, noise,
                       (uint32_t)seed, (uint32_t)(seed >> 32), c2, c3, L, total, noisy_n, x_t, combine);
  return se_check_launch("se_diffuse_noise");
}

// One workgroup, after the update in stream order: every lane reads n before lane 0 replaces it.
__global__ __launch_bounds__(SP_EMB) void sampler_advance_kernel(int* __restrict__ n_ptr, unsigned* __restrict__ run_ptr, int steps,
                                                                 const float* __restrict__ emb, float* __restrict__ d) {
  const int cur = *n_ptr;
  const bool wrap = cur <= 0 || cur >= steps;             // 0: the utterance is done; out of range: back to a valid state
  const int next = wrap ? steps - 1 : cur - 1;
  __syncthreads();
  if (threadIdx.x == 0) {
    *n_ptr = next;
    if (cur == 0) *run_ptr = *run_ptr + 1u;
  }
  d[threadIdx.x] = emb[(size_t)next * SP_EMB + threadIdx.x];
}

extern "C" int se_sampler_advance(int* n, unsigned* run, int steps, const float* emb, float* d, void* stream) {
  SE_REQUIRE(n && run && emb && d, "sampler_advance: null operand");
  SE_REQUIRE(steps > 0, "sampler_advance: bad step count %d", steps);
  hipLaunchKernelGGL(sampler_advance_kernel, dim3(1), dim3(SP_EMB), 0, as_stream(stream), n, run, steps, emb, d);
  return se_check_launch("se_sampler_advance");
}

__global__ __launch_bounds__(SP_THREADS) void sampler_begin_kernel(const float* __restrict__ x, const float* __restrict__ c,
                                                                   float* __restrict__ audio, float* __restrict__ noisy, int length,
                                                                   int padded) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * SP_THREADS + threadIdx.x;
  if (i >= padded) return;
  const float v = x[(size_t)b * length + (i < length ? i : i - length)] * c[b];       // the padded tail repeats the head
  audio[(size_t)b * padded + i] = v;
  noisy[(size_t)b * padded + i] = v;
}

extern "C" int se_sampler_begin(const float* x, const float* c, float* audio, float* noisy, int B, int length, int padded,
                                void* stream) {
  SE_REQUIRE(x && c && audio && noisy, "sampler_begin: null operand");
  SE_REQUIRE(B > 0 && B <= 65535 && length > 0 && padded >= length && padded - length <= length,
             "sampler_begin: bad sizes (B %d, length %d, padded %d)", B, length, padded);
  hipLaunchKernelGGL(sampler_begin_kernel, dim3((padded + SP_THREADS - 1) / SP_THREADS, B), dim3(SP_THREADS), 0, as_stream(stream), x,
                     c, audio, noisy, length, padded);
  return se_check_launch("se_sampler_begin");
}
