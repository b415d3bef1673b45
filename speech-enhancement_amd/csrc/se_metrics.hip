// Objective speech-quality measures of the reference's utils/compute_metrics.py on the device, all arithmetic in fp64
// (the reference is numpy fp64; an order-16 Levinson recursion and a log of a ratio of quadratic forms leave no room for fp32):
//
//   se_metric_frames        : WSS, LLR and segmental SNR of every 480-sample frame (skip 120) -- one workgroup per (utterance, frame):
//                             both frames are windowed once into LDS; segSNR with its clamps; autocorrelation lags 0..16 ->
//                             Levinson-Durbin -> LLR; ONE 1024-point complex FFT in LDS carries both real frames (clean = Re,
//                             processed = Im, separated by the conjugate symmetry) -> power spectrum bins 0..511 -> 25 critical-band
//                             energies in dB -> slopes, nearest-peak search, Klatt weights -> WSS
//   se_metric_trimmed_means : mean of the lowest round(0.95 n) values (WSS, LLR) and the plain mean (segSNR) by rank counting,
//                             one workgroup per (utterance, measure) -- no sort, no host round trip
//   se_metric_stoi          : six launches: polyphase resampling 16 kHz -> 10 kHz (up 5, down 8, 161-tap FIR), energies of the
//                             256-sample frames, the 40 dB silent-frame mask and its compaction (ballot prefix sums), the
//                             overlap-add of the kept frames gathered straight into the short-time DFT (512-point LDS FFT of
//                             the clean / processed pair) and its 15 third-octave bands, the clipped correlation over 30 frames,
//                             the mean
//
// A batch is B utterances of different lengths packed into one flat buffer per signal and described by the table `meta`
// (SE_METRIC_META int64 per utterance, include/se_hip.h).  The constant tables (windows, twiddles, filters) come from the host.
// Nothing here needs the matrix cores: a 10 s utterance is ~1300 + ~800 independent frames of a few thousand flops each.
#include "se_common.h"

constexpr int MT_WIN = 480, MT_SKIP = 120, MT_NFFT = 1024, MT_HALF = 512, MT_P = 16, MT_NCRIT = 25;
constexpr int ST_N = 256, ST_HOP = 128, ST_K = 512, ST_BINS = 257, ST_J = 15, ST_SEG = 30, ST_TAPS = 161;
constexpr int MM = SE_METRIC_META;
enum { M_OFF = 0, M_LEN, M_FOFF, M_NFR, M_ROFF, M_NR, M_SOFF, M_NSF, M_PROMOTE };

struct cplx { double x, y; };

// radix-2 decimation-in-time FFT of 2^LOG points held bit-reversed in LDS; tw[k] = exp(-2 pi i k / 1024), k < 512
template <int LOG>
static __device__ __forceinline__ void fft_lds(cplx* z, const cplx* __restrict__ tw, int tid, int nthr) {
  constexpr int N = 1 << LOG;
  for (int s = 0; s < LOG; ++s) {
    const int half = 1 << s;
    for (int b = tid; b < N / 2; b += nthr) {
      const int pos = b & (half - 1), i = ((b >> s) << (s + 1)) + pos, j = i + half;
      const cplx w = tw[pos << (9 - s)];
      const cplx a = z[i], c = z[j];
      const double tr = c.x * w.x - c.y * w.y, ti = c.x * w.y + c.y * w.x;
      z[j] = {a.x - tr, a.y - ti};
      z[i] = {a.x + tr, a.y + ti};
    }
    __syncthreads();
  }
}

static __device__ __forceinline__ double block_sum_256(double v, double* red, int tid) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// nearest spectral peak of band i (the reference's walk: `n < 24` to the right, `n >= 0` to the left, a zero slope goes left)
static __device__ __forceinline__ double loc_peak(const double* e, const double* sl, int i) {
  int n = i;
  if (sl[i] > 0) {
    while (n < MT_NCRIT - 1 && sl[n] > 0) ++n;
    return e[n - 1];
  }
  while (n >= 0 && sl[n] <= 0) --n;
  return e[n + 1];
}

__global__ __launch_bounds__(256) void metric_frames_kernel(const float* __restrict__ clean, const float* __restrict__ enh,
                                                            const long long* __restrict__ meta, const double* __restrict__ win,
                                                            const cplx* __restrict__ tw, const double* __restrict__ crit,
                                                            double* __restrict__ wss, double* __restrict__ llr,
                                                            double* __restrict__ snr) {
  __shared__ cplx z[MT_NFFT];
  __shared__ double fc[MT_WIN], fp[MT_WIN], pc[MT_HALF], pp[MT_HALF];
  __shared__ double R[2][MT_P + 1], lp[2][MT_P + 1], apast[2][MT_P], ec[MT_NCRIT], ep[MT_NCRIT], sc[MT_NCRIT - 1], sp[MT_NCRIT - 1],
      wt[MT_NCRIT - 1], wd[MT_NCRIT - 1], red[4];
  const long long* m = meta + (long)blockIdx.y * MM;
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (f >= (int)m[M_NFR]) return;
  const long base = m[M_OFF] + (long)f * MT_SKIP;                     // f * 120 + 480 <= length by the frame count
  const double add = m[M_PROMOTE] ? 0x1p-52 : 0.0;
  for (int n = tid; n < MT_NFFT; n += 256) {
    double c = 0.0, p = 0.0;
    if (n < MT_WIN) {
      const double w = win[n];
      c = ((double)clean[base + n] + add) * w;
      p = ((double)enh[base + n] + add) * w;
      fc[n] = c;
      fp[n] = p;
    }
    z[__brev((unsigned)n) >> 22] = {c, p};
  }
  __syncthreads();
  // segmental SNR
  double se = 0.0, ne = 0.0;
  for (int n = tid; n < MT_WIN; n += 256) {
    const double d = fc[n] - fp[n];
    se += fc[n] * fc[n];
    ne += d * d;
  }
  se = block_sum_256(se, red, tid);
  ne = block_sum_256(ne, red, tid);
  if (tid == 0) {
    const double eps = 0x1p-52;
    double v = 10.0 * log10(se / (ne + eps) + eps);
    v = v < -10.0 ? -10.0 : v;                                         // max(v, MIN_SNR) then min(., MAX_SNR); NaN passes through
    v = v > 35.0 ? 35.0 : v;
    snr[m[M_FOFF] + f] = v;
  }
  // autocorrelation lags 0..16 of both frames: 34 dot products over the four waves
  for (int q = wave; q < 2 * (MT_P + 1); q += 4) {
    const double* x = q <= MT_P ? fc : fp;
    const int k = q <= MT_P ? q : q - (MT_P + 1);
    double s = 0.0;
    for (int n = lane; n < MT_WIN - k; n += 64) s += x[n] * x[n + k];
    s = wave_sum_d(s);
    if (lane == 0) R[q <= MT_P ? 0 : 1][k] = s;
  }
  __syncthreads();
  // Levinson-Durbin, one lane per signal (waves 0 and 1); every array lives in LDS
  if (lane == 0 && wave < 2) {
    const double* r = R[wave];
    double* a = lp[wave] + 1;
    double* ap = apast[wave];
    double E = r[0];
    for (int i = 0; i < MT_P; ++i) {
      double s = 0.0;
      for (int k = 0; k < i; ++k) {
        ap[k] = a[k];
        s += ap[k] * r[i - k];
      }
      const double rc = (r[i + 1] - s) / E;
      a[i] = rc;
      for (int k = 0; k < i; ++k) a[k] = ap[k] - ap[i - 1 - k] * rc;
      E = (1.0 - rc * rc) * E;
    }
    lp[wave][0] = 1.0;
    for (int k = 0; k < MT_P; ++k) a[k] = -a[k];
  }
  // the FFT runs meanwhile on all threads (its barriers also publish lp)
  fft_lds<10>(z, tw, tid, 256);
  if (tid < 2) {                                                       // A toeplitz(R_clean) A for the processed / the clean model
    const double* A = lp[1 - tid];
    double q = 0.0;
    for (int j = 0; j <= MT_P; ++j) {
      double s = 0.0;
      for (int i = 0; i <= MT_P; ++i) s += A[i] * R[0][i > j ? i - j : j - i];
      q += s * A[j];
    }
    red[tid] = q;
  }
  // power spectra of the two real frames out of the one complex transform; frames were not divided by 32768: 2^-30 on the power
  for (int k = tid; k < MT_HALF; k += 256) {
    const cplx a = z[k], b = z[(MT_NFFT - k) & (MT_NFFT - 1)];
    const double cr = 0.5 * (a.x + b.x), ci = 0.5 * (a.y - b.y), pr = 0.5 * (a.y + b.y), pi = 0.5 * (b.x - a.x);
    pc[k] = (cr * cr + ci * ci) * 0x1p-30;
    pp[k] = (pr * pr + pi * pi) * 0x1p-30;
  }
  __syncthreads();
  if (tid == 0) llr[m[M_FOFF] + f] = log(red[0] / red[1]);
  // 25 critical-band energies in dB for both spectra
  for (int q = wave; q < 2 * MT_NCRIT; q += 4) {
    const int band = q < MT_NCRIT ? q : q - MT_NCRIT;
    const double* P = q < MT_NCRIT ? pc : pp;
    const double* F = crit + band * MT_HALF;
    double s = 0.0;
    for (int k = lane; k < MT_HALF; k += 64) s += F[k] * P[k];
    s = wave_sum_d(s);
    if (lane == 0) (q < MT_NCRIT ? ec : ep)[band] = 10.0 * log10(s > 1e-10 ? s : 1e-10);
  }
  __syncthreads();
  if (tid < MT_NCRIT - 1) {
    sc[tid] = ec[tid + 1] - ec[tid];
    sp[tid] = ep[tid + 1] - ep[tid];
  }
  __syncthreads();
  if (tid < MT_NCRIT - 1) {
    double mc = ec[0], mp = ep[0];
    for (int k = 1; k < MT_NCRIT; ++k) {
      mc = ec[k] > mc ? ec[k] : mc;
      mp = ep[k] > mp ? ep[k] : mp;
    }
    const double wc = (20.0 / (20.0 + mc - ec[tid])) * (1.0 / (1.0 + loc_peak(ec, sc, tid) - ec[tid]));
    const double wp = (20.0 / (20.0 + mp - ep[tid])) * (1.0 / (1.0 + loc_peak(ep, sp, tid) - ep[tid]));
    const double w = (wc + wp) / 2.0, d = sc[tid] - sp[tid];
    wt[tid] = w;
    wd[tid] = w * (d * d);
  }
  __syncthreads();
  if (tid == 0) {
    double num = 0.0, den = 0.0;
    for (int k = 0; k < MT_NCRIT - 1; ++k) {
      num += wd[k];
      den += wt[k];
    }
    wss[m[M_FOFF] + f] = num / den;
  }
}

// a sorts before b the way numpy sorts: ascending, NaN last; ties by index
static __device__ __forceinline__ bool sorts_before(double a, int ia, double b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na || nb) return na == nb ? ia < ib : nb;
  return a < b || (a == b && ia < ib);
}

__global__ __launch_bounds__(256) void metric_trimmed_kernel(const double* __restrict__ wss, const double* __restrict__ llr,
                                                             const double* __restrict__ snr, const long long* __restrict__ meta,
                                                             double* __restrict__ out) {
  __shared__ double red[4];
  const long long* m = meta + (long)blockIdx.y * MM;
  const int which = blockIdx.x, tid = threadIdx.x, n = (int)m[M_NFR];
  const double* a = (which == 0 ? wss : which == 1 ? llr : snr) + m[M_FOFF];
  const int keep = which == 2 ? n : (int)rint((double)n * 0.95);      // Python's round(): half to even
  double s = 0.0;
  for (int i = tid; i < n; i += 256) {
    const double v = a[i];
    bool in = true;
    if (keep < n) {
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += sorts_before(a[j], j, v, i) ? 1 : 0;
      in = rank < keep;
    }
    if (in) s += v;
  }
  s = block_sum_256(s, red, tid);
  if (tid == 0) out[blockIdx.y * 3 + which] = keep > 0 ? s / (double)keep : (double)NAN;
}

// ---- STOI ----
// out[j] = sum_i h[8 j + 80 - 5 i] x[i]: scipy's resample_poly(x, 5, 8) with its centring; taps visited with ascending i like its
// polyphase loop.  A float32 signal is filtered in float32 (taps and running sum, one rounding per product and per sum) because
// that is what scipy does for float32 input; a promoted (fp64) signal in fp64.  fir: [2][161], row 0 = the float32 taps.
__global__ __launch_bounds__(256) void stoi_resample_kernel(const float* __restrict__ clean, const float* __restrict__ enh,
                                                            const long long* __restrict__ meta, const double* __restrict__ fir,
                                                            double* __restrict__ xr, double* __restrict__ yr) {
  const long long* m = meta + (long)blockIdx.y * MM;
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= m[M_NR]) return;
  const long L = m[M_LEN], top = 8 * j + 80;
  long lo = (top - (ST_TAPS - 1) + 4) / 5, hi = top / 5;               // 0 <= top - 5 i <= 160
  if (top - (ST_TAPS - 1) < 0) lo = 0;
  if (hi > L - 1) hi = L - 1;
  const float* x = clean + m[M_OFF];
  const float* y = enh + m[M_OFF];
  if (m[M_PROMOTE]) {
    const double* h = fir + ST_TAPS;
    double ax = 0.0, ay = 0.0;
    for (long i = lo; i <= hi; ++i) {
      const double t = h[top - 5 * i];
      ax += ((double)x[i] + 0x1p-52) * t;
      ay += ((double)y[i] + 0x1p-52) * t;
    }
    xr[m[M_ROFF] + j] = ax;
    yr[m[M_ROFF] + j] = ay;
  } else {
    float ax = 0.f, ay = 0.f;
    for (long i = lo; i <= hi; ++i) {
      const float t = (float)fir[top - 5 * i];
      ax = __fadd_rn(ax, __fmul_rn(x[i], t));
      ay = __fadd_rn(ay, __fmul_rn(y[i], t));
    }
    xr[m[M_ROFF] + j] = (double)ax;
    yr[m[M_ROFF] + j] = (double)ay;
  }
}

// energy in dB of the clean frame x[start - 1 : start + 255] * w (the reference's shifted index; -1 of frame 0 wraps to the end)
__global__ __launch_bounds__(64) void stoi_energy_kernel(const double* __restrict__ xr, const long long* __restrict__ meta,
                                                         const double* __restrict__ hann, double* __restrict__ energy) {
  const long long* m = meta + (long)blockIdx.y * MM;
  const int j = blockIdx.x, lane = threadIdx.x;
  if (j >= (int)m[M_NSF]) return;
  const double* x = xr + m[M_ROFF];
  const long nr = m[M_NR];
  double s = 0.0;
  for (int k = lane; k < ST_N; k += 64) {
    long i = (long)j * ST_HOP - 1 + k;                                 // start + 255 <= nr - 1 by the frame count
    if (i < 0) i = nr - 1;
    const double v = x[i] * hann[k];
    s += v * v;
  }
  s = wave_sum_d(s);
  if (lane == 0) energy[m[M_SOFF] + j] = 20.0 * log10(sqrt(s) / 16.0);
}

// mask = energy - max + 40 > 0; kept[] = indices of the surviving frames in order, count[b] = their number
__global__ __launch_bounds__(256) void stoi_mask_kernel(const double* __restrict__ energy, const long long* __restrict__ meta,
                                                        int* __restrict__ kept, int* __restrict__ count) {
  __shared__ double redm[4];
  __shared__ int wtot[4];
  const long long* m = meta + (long)blockIdx.x * MM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nsf = (int)m[M_NSF];
  const double* e = energy + m[M_SOFF];
  int* kp = kept + m[M_SOFF];
  double mx = -INFINITY;
  bool bad = false;
  for (int j = tid; j < nsf; j += 256) {
    const double v = e[j];
    bad |= v != v;
    mx = v > mx ? v : mx;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double t = __shfl_xor(mx, o, 64);
    mx = t > mx ? t : mx;
  }
  bad = __any(bad);
  if (lane == 0) redm[wave] = bad ? (double)NAN : mx;
  __syncthreads();
  mx = redm[0];
  for (int w = 1; w < 4; ++w) mx = (redm[w] > mx || redm[w] != redm[w]) ? redm[w] : mx;      // np.max propagates NaN
  int base = 0;
  for (int j0 = 0; j0 < nsf; j0 += 256) {
    const int j = j0 + tid;
    const bool on = j < nsf && (e[j < nsf ? j : 0] - mx + 40.0) > 0.0;
    const unsigned long long bal = __ballot(on);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    int woff = 0, tot = 0;
    for (int w = 0; w < 4; ++w) {
      woff += w < wave ? wtot[w] : 0;
      tot += wtot[w];
    }
    if (on) kp[base + woff + before] = j;
    base += tot;
  }
  if (tid == 0) count[blockIdx.x] = base;
}

// short-time DFT frame f of the silence-free signals: sample n of output slot c comes from kept frame c (overlap-add of at most two
// windowed frames, the earlier one first), windowed again, 512-point transform of the (clean, processed) pair, 15 band magnitudes
__global__ __launch_bounds__(256) void stoi_bands_kernel(const double* __restrict__ xr, const double* __restrict__ yr,
                                                         const long long* __restrict__ meta, const int* __restrict__ kept,
                                                         const int* __restrict__ count, const double* __restrict__ hann,
                                                         const cplx* __restrict__ tw, const double* __restrict__ H,
                                                         double scale2, double* __restrict__ X, double* __restrict__ Y) {
  __shared__ cplx z[ST_K];
  __shared__ double px[ST_BINS], py[ST_BINS];
  const int b = blockIdx.y, f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long* m = meta + (long)b * MM;
  const int cnt = count[b];
  if (f >= cnt - 1) return;                                            // stdft keeps int((len - 256) / 128) = count - 1 frames
  const double* x = xr + m[M_ROFF];
  const double* y = yr + m[M_ROFF];
  const int* kp = kept + m[M_SOFF];
  {
    const int n = tid, pos = f * ST_HOP + n, c0 = pos / ST_HOP;
    double vx = 0.0, vy = 0.0;
    for (int c = c0 - 1; c <= c0; ++c) {
      if (c < 0 || c >= cnt) continue;
      const int k = pos - c * ST_HOP;                                  // 0 <= k < 256
      const long i = (long)kp[c] * ST_HOP + k;                         // < nr: frame starts stop before nr - 256
      vx += x[i] * hann[k];
      vy += y[i] * hann[k];
    }
    z[__brev((unsigned)n) >> 23] = {vx * hann[n], vy * hann[n]};
    z[__brev((unsigned)(n + ST_N)) >> 23] = {0.0, 0.0};
  }
  __syncthreads();
  fft_lds<9>(z, tw, tid, 256);
  for (int k = tid; k < ST_BINS; k += 256) {
    const cplx a = z[k], c = z[(ST_K - k) & (ST_K - 1)];
    const double cr = 0.5 * (a.x + c.x), ci = 0.5 * (a.y - c.y), pr = 0.5 * (a.y + c.y), pi = 0.5 * (c.x - a.x);
    px[k] = (cr * cr + ci * ci) * scale2;
    py[k] = (pr * pr + pi * pi) * scale2;
  }
  __syncthreads();
  for (int q = wave; q < 2 * ST_J; q += 4) {
    const int band = q < ST_J ? q : q - ST_J;
    const double* P = q < ST_J ? px : py;
    double s = 0.0;
    for (int k = lane; k < ST_BINS; k += 64) s += H[band * ST_BINS + k] * P[k];
    s = wave_sum_d(s);
    if (lane == 0) (q < ST_J ? X : Y)[(m[M_SOFF] + f) * ST_J + band] = sqrt(s);
  }
}

// intermediate intelligibility d[i] of the 30-frame segment that starts at frame i: one wave, lane = frame of the segment
__global__ __launch_bounds__(64) void stoi_dinterm_kernel(const double* __restrict__ X, const double* __restrict__ Y,
                                                          const long long* __restrict__ meta, const int* __restrict__ count,
                                                          double* __restrict__ d) {
  const int b = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
  const long long* m = meta + (long)b * MM;
  if (i + ST_SEG > count[b] - 1) return;
  const bool on = lane < ST_SEG;
  const long row = (m[M_SOFF] + i + (on ? lane : 0)) * ST_J;
  const double clip = pow(10.0, 15.0 / 20.0);
  double acc = 0.0;
  for (int j = 0; j < ST_J; ++j) {
    const double x = on ? X[row + j] : 0.0, y = on ? Y[row + j] : 0.0;
    const double alpha = sqrt(wave_sum_d(x * x) / wave_sum_d(y * y));
    const double ay = y * alpha, xc = x + x * clip;
    const double yp = xc < ay ? xc : ay;
    const double mx = wave_sum_d(x) / ST_SEG, my = wave_sum_d(on ? yp : 0.0) / ST_SEG;
    const double xn = on ? x - mx : 0.0, yn = on ? yp - my : 0.0;
    const double nx = sqrt(wave_sum_d(xn * xn)), ny = sqrt(wave_sum_d(yn * yn));
    acc += wave_sum_d(on ? (xn / nx) * (yn / ny) : 0.0);
  }
  if (lane == 0) d[m[M_SOFF] + i] = acc / ST_J;
}

__global__ __launch_bounds__(256) void stoi_mean_kernel(const double* __restrict__ d, const long long* __restrict__ meta,
                                                        const int* __restrict__ count, double* __restrict__ out) {
  __shared__ double red[4];
  const long long* m = meta + (long)blockIdx.x * MM;
  const int tid = threadIdx.x, n = count[blockIdx.x] - 1 - (ST_SEG - 1);
  double s = 0.0;
  for (int i = tid; i < n; i += 256) s += d[m[M_SOFF] + i];
  s = block_sum_256(s, red, tid);
  if (tid == 0) out[blockIdx.x] = n > 0 ? s / (double)n : (double)NAN;   // fewer than 30 frames: the mean of nothing
}

static inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

extern "C" size_t se_metric_stoi_workspace_bytes(long total_resampled, long total_frames, int B) {
  if (total_resampled < 0 || total_frames < 0 || B <= 0) return 0;
  return 2 * al256((size_t)total_resampled * 8) + al256((size_t)total_frames * 8) + al256((size_t)total_frames * 4) +
         2 * al256((size_t)total_frames * ST_J * 8) + 256;
}

extern "C" int se_metric_frames(const float* clean, const float* enh, const long long* meta, int B, int max_frames,
                                const double* window, const double* twiddle, const double* crit_filter, double* wss, double* llr,
                                double* snr, void* stream) {
  SE_REQUIRE(clean && enh && meta && window && twiddle && crit_filter && wss && llr && snr, "metric_frames: null operand");
  SE_REQUIRE(B > 0 && B <= 65535 && max_frames >= 0, "metric_frames: bad batch (%d) or frame count (%d)", B, max_frames);
  if (max_frames == 0) return 0;
  hipLaunchKernelGGL(metric_frames_kernel, dim3(max_frames, B), dim3(256), 0, as_stream(stream), clean, enh, meta, window,
                     reinterpret_cast<const cplx*>(twiddle), crit_filter, wss, llr, snr);
  return se_check_launch("se_metric_frames");
}

extern "C" int se_metric_trimmed_means(const double* wss, const double* llr, const double* snr, const long long* meta, int B,
                                       double* out, void* stream) {
  SE_REQUIRE(wss && llr && snr && meta && out, "metric_trimmed_means: null operand");
  SE_REQUIRE(B > 0 && B <= 65535, "metric_trimmed_means: bad batch (%d)", B);
  hipLaunchKernelGGL(metric_trimmed_kernel, dim3(3, B), dim3(256), 0, as_stream(stream), wss, llr, snr, meta, out);
  return se_check_launch("se_metric_trimmed_means");
}

extern "C" int se_metric_stoi(const float* clean, const float* enh, const long long* meta, int B, long total_resampled,
                              long total_frames, int max_resampled, int max_frames, const double* fir, const double* hann,
                              const double* twiddle, const double* thirdoct, void* workspace, size_t workspace_bytes,
                              double* d_interm, int* count, double* out, void* stream) {
  SE_REQUIRE(clean && enh && meta && fir && hann && twiddle && thirdoct && d_interm && count && out, "metric_stoi: null operand");
  SE_REQUIRE(B > 0 && B <= 65535 && max_resampled >= 0 && max_frames >= 0, "metric_stoi: bad batch (%d) or sizes", B);
  SE_REQUIRE(workspace && workspace_bytes >= se_metric_stoi_workspace_bytes(total_resampled, total_frames, B),
             "metric_stoi: workspace of %zu bytes is too small", workspace_bytes);
  char* p = (char*)(((size_t)workspace + 255) & ~(size_t)255);
  double* xr = (double*)p;       p += al256((size_t)total_resampled * 8);
  double* yr = (double*)p;       p += al256((size_t)total_resampled * 8);
  double* energy = (double*)p;   p += al256((size_t)total_frames * 8);
  int* kept = (int*)p;           p += al256((size_t)total_frames * 4);
  double* X = (double*)p;        p += al256((size_t)total_frames * ST_J * 8);
  double* Y = (double*)p;
  hipStream_t s = as_stream(stream);
  const cplx* tw = reinterpret_cast<const cplx*>(twiddle);
  double wsum = 0.0;                                                   // scipy.signal.stft scales by 1 / sum(window)
  for (int k = 1; k <= ST_N; ++k) wsum += 0.5 - 0.5 * cos(2.0 * 3.14159265358979323846 * k / (ST_N + 1));
  if (max_resampled > 0)
    hipLaunchKernelGGL(stoi_resample_kernel, dim3(cdiv(max_resampled, 256), B), dim3(256), 0, s, clean, enh, meta, fir, xr, yr);
  if (max_frames > 0) hipLaunchKernelGGL(stoi_energy_kernel, dim3(max_frames, B), dim3(64), 0, s, xr, meta, hann, energy);
  hipLaunchKernelGGL(stoi_mask_kernel, dim3(B), dim3(256), 0, s, energy, meta, kept, count);
  if (max_frames > 1) {
    hipLaunchKernelGGL(stoi_bands_kernel, dim3(max_frames - 1, B), dim3(256), 0, s, xr, yr, meta, kept, count, hann, tw, thirdoct,
                       1.0 / (wsum * wsum), X, Y);
    if (max_frames > ST_SEG)
      hipLaunchKernelGGL(stoi_dinterm_kernel, dim3(max_frames - ST_SEG, B), dim3(64), 0, s, X, Y, meta, count, d_interm);
  }
  hipLaunchKernelGGL(stoi_mean_kernel, dim3(B), dim3(256), 0, s, d_interm, meta, count, out);
  return se_check_launch("se_metric_stoi");
}
