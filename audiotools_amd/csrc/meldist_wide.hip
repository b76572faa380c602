// Fused mel-spectrogram distance for gfx950, WIDE filterbanks: n_fft/4 < n_mels <= min(2 n_fft, 512) on windows 32 ... 1024.
//
// mel_dist_kernel (meldist.hip) keeps the target's bands in registers: band m of a frame belongs to lane m % L and a lane
// has room for 8 of them, hence n_mels <= n_fft/4.  Recipes with one filterbank size at every scale (64 bands on windows
// 64 ... 2048, 80 or 128 bands on 256) exceed that on their small windows.  This kernel computes the same sums, the same G
// and the same dx with the target's bands PARKED IN LDS and a band walk of run-time length.
//
// Design (CDNA4).  Shared with mel_dist_kernel (the frame loader and the transform below are restated from it, arithmetic
// unchanged): the wave FFT of fft_wave.h, M = n_fft/2 complex points, 16 per lane, L = M/16 lanes per frame, FW = 64/L
// frames per wave; a persistent grid, one contiguous run of frame groups per wave; reflect margins by index arithmetic; y
// and x frames of a group loaded together; two float accumulators per lane, one partial pair per wave, a one-workgroup
// finalize in double; no atomics.  What differs:
//  * band row: every wave owns FW x n_mels floats of dynamic LDS, sized from the launch's n_mels (at the cap of every
//    window FW n_mels <= 4096 floats = 16 KB per wave; at (256, 80) 640 floats).  Slot fs n_mels + m belongs to lane
//    m % L of frame slot fs in every stage: it is lane-private, no exchange point guards it;
//  * y stage: |Y| goes into the frame's slab in bin order; lane t walks bands t, t + L, t + 2L, ... < n_mels (bins
//    ascending, one fmaf per bin from 0, four independent LDS loads per step -- the summation order of mel_dist_kernel)
//    and stores mel_y[m] in the row.  Nothing of the target stays in registers across x's transform;
//  * x stage: |X| into the slab, the same walk; the lane reads mel_y[m] back, forms both log terms (v_log_f32, the clamp on
//    mel itself), adds to its accumulators and, in the gradient modes, overwrites the slot with dL/dmel[m].  An all-zero
//    band (span count 0) has mel = 0 on both sides: both differences and the gradient are exactly 0;
//  * back-projection, G store and the DIST_DX tail read dL/dmel from the band row; band indices and spans are clamped, so
//    that no table can address outside the workgroup's LDS.
#include "at_common.h"
#include "fft_wave.h"
#include "dist_ola.h"
#include <float.h>

extern "C" int at_stft_fused_supported(int n_fft);

namespace {

constexpr int NW = 4;              // waves per workgroup
constexpr int MAX_BLOCKS = 1024;   // persistent grid bound the workspace is sized for
constexpr int MAX_MELS = 512;      // band indices travel in 16 bits; FW n_mels <= 4096 at every window
constexpr int LDS_CU = 160 * 1024; // LDS of a compute unit (and the most one workgroup may ask for)

struct WideArgs {
  const float* x;          // (rows, T) estimate
  const float* y;          // (rows, T) target
  const float* window;     // (n_fft)
  const float2* tw;        // (n_fft): (cos, -sin)(2 pi k / n_fft)
  const int* bin_bands;    // (M + 1): lo | hi << 16
  const float2* bin_w;     // (M + 1): weights of lo and hi (0 where absent)
  const int* band_span;    // (n_mels): first bin | count << 16
  float2* G;               // (rows, n_out, M+1) or null
  float2* partials;        // (gridDim.x * NW) {sum log, sum mag}
  int T;
  int n_out;               // frames per row
  int hop;
  int gpr;                 // frame groups per row: ceil(n_out / FW)
  int64_t total_groups;    // rows * gpr
  int n_mels;
  float eps;               // clamp of mel (not of its square)
  float c_log;             // power * log10(2):  c_log * log2(mel) = power * log10 mel
  float g_logp;            // g_log * power / ln 10   (LOSS_L2: times 2, and so is g_mag)
  float g_mag;
  int vec2;                // rows of x and y are 8-byte aligned: float2 loads
  OlaOut ola;              // DIST_DX only: where the waveform gradient goes (dist_ola.h)
};

// LDS (floats): [NW wave slabs][window, halved: 2M][split twiddles: M][pass-2 twiddles: 16 x 36]   (as mel_dist_kernel)
//               [bin weights: 2 (M+1)][bin bands: M+1][DIST_DX: NW carries of the overlap-add, 24 L floats each]
//               [band spans: n_mels][NW band rows: FW n_mels each]            <- sized at launch
template <int M>
constexpr int fixed_floats(int mode) {
  return NW * 2 * WAVE_LDS_SLOTS + 2 * M + M + 16 * 36 + 3 * (M + 1) + (mode == DIST_DX ? NW * ola_carry_floats<M>() : 0);
}
constexpr int row_floats(int M, int n_mels) { return n_mels + NW * (64 / (M / 16)) * n_mels; }

// bytes of a launch at run-time M (the fixed part as fixed_floats<M>)
int64_t lds_bytes(int M, int n_mels, bool dx) {
  return 4 * (int64_t)(NW * 2 * WAVE_LDS_SLOTS + 3 * M + 16 * 36 + 3 * (M + 1) + (dx ? NW * 3 * (M / 2) : 0) + row_floats(M, n_mels));
}

__device__ __forceinline__ float abs2(float2 z) { return fmaf(z.x, z.x, z.y * z.y); }
__device__ __forceinline__ float sgnf(float a, float b) { return (a > b ? 1.f : 0.f) - (a < b ? 1.f : 0.f); }

template <int M, int MODE, int LOSS>
__global__ __launch_bounds__(NW * 64, 2) void mel_dist_wide_kernel(const WideArgs A) {
  constexpr bool GRAD = MODE != DIST_NONE;
  using P = Plan<M>;
  constexpr int L = P::L, FW = P::FW, N = 2 * M, F = M + 1;
  extern __shared__ __attribute__((aligned(16))) float lds_f[];
  float* s_win = lds_f + NW * 2 * WAVE_LDS_SLOTS;
  float2* s_twp = reinterpret_cast<float2*>(s_win + N);
  float* s_tw2 = s_win + N + M;
  float2* s_bw = reinterpret_cast<float2*>(s_tw2 + 16 * 36);       // an even number of floats in: 8-byte aligned
  int* s_bb = reinterpret_cast<int*>(s_tw2 + 16 * 36 + 2 * F);
  float* s_carry = reinterpret_cast<float*>(s_bb + F);
  int* s_span = reinterpret_cast<int*>(s_carry + (MODE == DIST_DX ? NW * ola_carry_floats<M>() : 0));
  const int n_mels = __builtin_amdgcn_readfirstlane(A.n_mels);
  float* s_rows = reinterpret_cast<float*>(s_span + n_mels);
  // the factor 1/2 of the split step rides on the window (exact in binary floating point)
  for (int i = threadIdx.x; i < N; i += NW * 64) s_win[i] = 0.5f * A.window[i];
  for (int i = threadIdx.x; i < M / 2; i += NW * 64) s_twp[i] = A.tw[i];
  if constexpr (P::R2 > 1) {
    for (int i = threadIdx.x; i < 16 * P::R2; i += NW * 64) {
      const int jj = i / P::R2, r = i % P::R2;
      reinterpret_cast<float2*>(s_tw2 + jj * 36)[r] = A.tw[r * jj * (N / (16 * P::R2))];
    }
  }
  for (int i = threadIdx.x; i < F; i += NW * 64) {
    s_bw[i] = A.bin_w[i];
    s_bb[i] = A.bin_bands[i];
  }
  // a span never leaves the F bins whatever the table says
  for (int i = threadIdx.x; i < n_mels; i += NW * 64) {
    const int sp = A.band_span[i];
    const int k0 = min(sp & 0xffff, F);
    const int cnt = min((sp >> 16) & 0x7fff, F - k0);
    s_span[i] = k0 | (cnt << 16);
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fs = lane / L;  // frame slot inside the wave
  const int t = lane % L;   // thread inside the frame
  float2* wbuf = reinterpret_cast<float2*>(lds_f) + wave * WAVE_LDS_SLOTS;
  float2* fbuf = wbuf + fs * P::SLOTS;
  float* fmag = reinterpret_cast<float*>(fbuf);           // |.| of the frame's F bins, in bin order (F <= 2 SLOTS floats)
  float* brow = s_rows + (wave * FW + fs) * n_mels;       // the frame's band row: mel_y, then dL/dmel
  float* carry = s_carry + wave * ola_carry_floats<M>();  // DIST_DX only: lane-private, element i is lane i % 64's
  if constexpr (MODE == DIST_DX) {
    for (int i = lane; i < ola_carry_floats<M>(); i += 64) carry[i] = 0.f;
  }

  constexpr int NB2 = 16 / P::R2;
  constexpr int NB3 = 16 / P::R3;
  float2 tw3b[P::R3 > 1 ? NB3 : 1];  // base twiddle per butterfly of pass 3; its powers are derived
  if constexpr (P::R3 > 1) {
    constexpr int NS = 16 * P::R2;
#pragma unroll
    for (int b = 0; b < NB3; ++b) tw3b[b] = A.tw[((t + b * L) % NS) * (N / (NS * P::R3))];
  }

  // ---- samples of this thread's frame: points t + L q of z[n] = s[2n] + i s[2n+1].  Interior frames load directly;
  // a group that touches a reflected margin takes a rolled loop through the wave's slab (index arithmetic, no copy).
  auto load_frame = [&](float2 (&a)[16], const float* __restrict__ sr, int s0, bool interior) __attribute__((always_inline)) {
    if (interior) {
      if (A.vec2) {
        const float2* __restrict__ p = reinterpret_cast<const float2*>(sr + s0);
#pragma unroll
        for (int q = 0; q < 16; ++q) a[q] = p[t + L * q];
      } else {
        const float* __restrict__ p = sr + s0;
#pragma unroll
        for (int q = 0; q < 16; ++q) a[q] = make_float2(p[2 * (t + L * q)], p[2 * (t + L * q) + 1]);
      }
    } else {
#pragma unroll 1
      for (int q = 0; q < 16; ++q) {
        const int n = t + L * q;
        int u0 = s0 + 2 * n, u1 = u0 + 1;          // centre reflect padding: one reflection (T > n_fft/2)
        u0 = u0 < 0 ? -u0 : u0; u0 = u0 >= A.T ? 2 * (A.T - 1) - u0 : u0;
        u1 = u1 < 0 ? -u1 : u1; u1 = u1 >= A.T ? 2 * (A.T - 1) - u1 : u1;
        u0 = min(max(u0, 0), A.T - 1); u1 = min(max(u1, 0), A.T - 1);
        fbuf[n] = make_float2(sr[u0], sr[u1]);
      }
      wave_sync();
#pragma unroll
      for (int q = 0; q < 16; ++q) a[q] = fbuf[t + L * q];
      wave_sync();
    }
  };

  // ---- window, M-point complex FFT, real-FFT split.  Out: bins k = t + L q in xa[q], bins M - k in xb[q] (thread 0,
  // q = 0: DC and Nyquist), bin M/2 in xh (thread 0 only; 0 elsewhere).  The slab is free again on return.
  auto transform = [&](float2 (&a)[16], float2 (&xa)[8], float2 (&xb)[8], float2& xh) __attribute__((always_inline)) {
    {
      const float2* w2 = reinterpret_cast<const float2*>(s_win);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float2 w = w2[t + L * q];
        a[q] = make_float2(a[q].x * w.x, a[q].y * w.y);
      }
    }
    pass_compute_store<16, 1, L>(a, fbuf, t, nullptr);
    wave_sync();
    if constexpr (P::R2 > 1) {
      load_points<L>(a, fbuf, t);
      wave_sync();
      float2 tw2[NB2 * P::R2];
#pragma unroll
      for (int b = 0; b < NB2; ++b) {
        const float2* rowp = reinterpret_cast<const float2*>(s_tw2 + ((t + b * L) & 15) * 36);
#pragma unroll
        for (int r = 1; r < P::R2; ++r) tw2[b * P::R2 + r] = rowp[r];
      }
      pass_compute_store<P::R2, 16, L>(a, fbuf, t, tw2);
      wave_sync();
    }
    if constexpr (P::R3 > 1) {
      load_points<L>(a, fbuf, t);
      wave_sync();
      float2 tw3[NB3 * P::R3];
#pragma unroll
      for (int b = 0; b < NB3; ++b) {
        tw3[b * P::R3 + 1] = tw3b[b];
#pragma unroll
        for (int r = 2; r < P::R3; ++r) tw3[b * P::R3 + r] = cmul(tw3[b * P::R3 + r - 1], tw3b[b]);
      }
      pass_compute_store<P::R3, 16 * P::R2, L>(a, fbuf, t, tw3);
      wave_sync();
    }
    float2 zh = make_float2(0.f, 0.f);
    if (t == 0) zh = fbuf[phys<L>(M / 2)];
    xh = make_float2(2.f * zh.x, -2.f * zh.y);       // k == M/2: X = conj(Z[M/2])  (Z carries the halved window)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int k = t + L * q;
      const float2 zk = fbuf[phys<L>(k)];
      const float2 zm = fbuf[phys<L>((M - k) & (M - 1))];
      if (q == 0 && t == 0) {   // packed point 0: DC and Nyquist, two real bins
        xa[q] = make_float2(2.f * (zk.x + zk.y), 0.f);
        xb[q] = make_float2(2.f * (zk.x - zk.y), 0.f);
      } else {
        const float2 twp = s_twp[k];  // (cos, -sin)(2 pi k / N)
        const float sr = zk.x + zm.x, si = zk.y - zm.y;
        const float dr = zk.x - zm.x, di = zk.y + zm.y;
        const float c = twp.x, s = -twp.y;
        const float pp = fmaf(s, dr, -c * di);
        const float qq = fmaf(s, di, c * dr);
        xa[q] = make_float2(sr - pp, si - qq);
        xb[q] = make_float2(sr + pp, -si - qq);
      }
    }
    wave_sync();
  };

  // ---- |.| of the frame's spectrum into its slab, in bin order
  auto put_mag = [&](const float2 (&xa)[8], const float2 (&xb)[8], float2 xh) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int k = t + L * q;
      fmag[k] = __builtin_amdgcn_sqrtf(abs2(xa[q]));
      fmag[M - k] = __builtin_amdgcn_sqrtf(abs2(xb[q]));
    }
    if (t == 0) fmag[M / 2] = __builtin_amdgcn_sqrtf(abs2(xh));
    wave_sync();
  };

  // ---- band m (< n_mels) of the frame from the magnitudes in its slab.  Summation order: the band's bins in ascending
  // order, s = fmaf(w, |.|, s) from s = 0 (the four loads of a step are independent, the adds are not reordered; a slot
  // past the span's end adds w = 0, which leaves s as it is).  An all-zero band (count 0) is 0.
  auto band = [&](int m) __attribute__((always_inline)) -> float {
    const int sp = s_span[m];
    const int k0 = sp & 0xffff, cnt = sp >> 16;
    float s = 0.f;
    for (int i = 0; i < cnt; i += 4) {
      float w[4], v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = min(k0 + i + u, M);
        const float2 ww = s_bw[k];
        const float wk = (s_bb[k] & 0xffff) == m ? ww.x : ww.y;
        w[u] = i + u < cnt ? wk : 0.f;
        v[u] = fmag[k];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) s = fmaf(w[u], v[u], s);
    }
    return s;
  };

  // ---- this wave's run of frame groups
  // (DIST_DX: only the first n_active <= total_groups waves own groups, so that no run is empty)
  const int64_t n_waves = MODE == DIST_DX ? (int64_t)A.ola.n_active : (int64_t)gridDim.x * NW;
  const int64_t gw = (int64_t)blockIdx.x * NW + wave;
  int64_t g_lo = A.total_groups * gw / n_waves;
  int64_t g_hi = A.total_groups * (gw + 1) / n_waves;
  if constexpr (MODE == DIST_DX) {
    if (gw >= n_waves) g_lo = g_hi = 0;
  }
  float s_log = 0.f, s_mag = 0.f;

  for (int64_t g = g_lo; g < g_hi; ++g) {
    const int64_t row = g / A.gpr;
    const int gb = (int)(g - row * A.gpr);
    const int f0 = gb * FW;
    const bool valid = f0 + fs < A.n_out;
    const int fo = min(f0 + fs, A.n_out - 1);     // slots past the row's last frame repeat it (and are masked below)
    const int s0 = fo * A.hop - M;                // first sample of the frame in un-padded coordinates
    const bool interior = __all(s0 >= 0 && s0 + N <= A.T);
    float2 ay[16], ax[16];
    load_frame(ay, A.y + row * A.T, s0, interior);
    load_frame(ax, A.x + row * A.T, s0, interior);

    // target: mel_y of the lane's bands goes to the band row
    {
      float2 xa[8], xb[8], xh;
      transform(ay, xa, xb, xh);
      put_mag(xa, xb, xh);
      for (int m = t; m < n_mels; m += L) brow[m] = band(m);
      wave_sync();                                 // the slab is free again
    }

    // estimate: X stays in registers until G is formed
    {
      float2 xa[8], xb[8], xh;
      transform(ax, xa, xb, xh);
      put_mag(xa, xb, xh);
      for (int m = t; m < n_mels; m += L) {
        const float a = band(m), b = brow[m];
        const float la = A.c_log * __builtin_amdgcn_logf(fmaxf(a, A.eps));
        const float lb = A.c_log * __builtin_amdgcn_logf(fmaxf(b, A.eps));
        if constexpr (LOSS == LOSS_L2) {
          // squared error: the differences take the place of their signs (A.g_logp and A.g_mag carry the factor 2); below
          // the clamp la is the constant p log10 eps, so the [a >= eps] select is all the clamp needs
          const float dl = la - lb, dm = a - b;
          s_log += valid ? dl * dl : 0.f;
          s_mag += valid ? dm * dm : 0.f;
          if constexpr (GRAD) {
            const float gl = a >= A.eps ? A.g_logp * dl * __builtin_amdgcn_rcpf(a) : 0.f;
            brow[m] = fmaf(A.g_mag, dm, gl);
          }
        } else {
          s_log += valid ? fabsf(la - lb) : 0.f;
          s_mag += valid ? fabsf(a - b) : 0.f;
          if constexpr (GRAD) {
            const float sl = sgnf(fmaxf(a, A.eps), fmaxf(b, A.eps));
            const float gl = a >= A.eps ? A.g_logp * sl * __builtin_amdgcn_rcpf(a) : 0.f;
            brow[m] = fmaf(A.g_mag, sgnf(a, b), gl);
          }
        }
      }
      wave_sync();                                 // the slab is free again; the row holds dL/dmel
      if constexpr (GRAD) {
        // back-projection onto the lane's bins; a slot of weight 0 adds exactly 0 whatever band index it carries
        auto gbin = [&](float2 X, int k) __attribute__((always_inline)) -> float2 {
          const float2 w = s_bw[k];
          const int bb = s_bb[k];
          const int lo = min(bb & 0xffff, n_mels - 1), hi = min((bb >> 16) & 0xffff, n_mels - 1);
          const float c0 = w.x != 0.f ? w.x * brow[lo] : 0.f;
          const float c = w.y != 0.f ? fmaf(w.y, brow[hi], c0) : c0;
          // 1/|X|; G = 0 where |X|^2 is zero (or below the normal range, where v_rsq_f32 is not defined)
          const float a2 = abs2(X);
          const float inv = a2 >= FLT_MIN ? __builtin_amdgcn_rsqf(a2) : 0.f;
          const float coef = c * inv;
          return make_float2(coef * X.x, coef * X.y);
        };
        float2* sx = fbuf;                           // G of frame slot fs, bins in order
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int k = t + L * q;
          sx[k] = gbin(xa[q], k);
          sx[M - k] = gbin(xb[q], M - k);
        }
        if (t == 0) sx[M / 2] = gbin(xh, M / 2);
        wave_sync();
      }
      if constexpr (MODE == DIST_DX) {
        // G stays on chip: adjoint transform of every frame, overlap-add inside the wave (dist_ola.h)
        ola_frame<M>(fbuf, wbuf, s_win, s_twp, s_tw2, tw3b, t, fs, valid);
        ola_group<M>(reinterpret_cast<const float*>(wbuf), carry, lane, A.ola, row, f0, gb == A.gpr - 1);
      }
      if constexpr (MODE == DIST_G) {
        // the FW frames of the group are consecutive rows of G: (M + 1) FW contiguous float2, streamed as 512-byte runs
        constexpr int TOT = FW * (M + 1);
        constexpr int NST = (TOT + 63) / 64;
        const int tot = min(FW, A.n_out - f0) * (M + 1);       // only the frames that exist
        float2* __restrict__ obase = A.G + (row * A.n_out + f0) * (M + 1);
#pragma unroll
        for (int i = 0; i < NST; ++i) {
          const int idx = i * 64 + lane;
          if (idx < tot) {
            const int f = idx / (M + 1);
            at::stg2<true>(obase + idx, wbuf[f * P::SLOTS + (idx - f * (M + 1))]);
          }
        }
        wave_sync();
      }
    }
  }
  if constexpr (MODE == DIST_DX) {
    if (g_hi > g_lo && g_hi % A.gpr != 0) {     // the run ends inside a row: its carry is the next wave's missing part
      for (int i = lane; i < ola_carry_floats<M>(); i += 64) A.ola.seams[gw * ola_carry_floats<M>() + i] = carry[i];
    }
  }
  s_log = at::wave_sum(s_log);
  s_mag = at::wave_sum(s_mag);
  if (lane == 0) A.partials[gw] = make_float2(s_log, s_mag);
}

// One workgroup: the partial pairs of all waves, added in double in a fixed order (thread i takes i, i + 256, ...; then a
// fixed tree), so that the same inputs give the same bits on every run.  The scheme of mel_dist_finalize, restated.
__global__ __launch_bounds__(256) void mel_dist_wide_finalize(const float2* __restrict__ partials, int n, double* __restrict__ sums) {
  __shared__ double sh[2][256];
  double s0 = 0.0, s1 = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float2 p = partials[i];
    s0 += (double)p.x;
    s1 += (double)p.y;
  }
  sh[0][threadIdx.x] = s0;
  sh[1][threadIdx.x] = s1;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    sums[0] = sh[0][0];
    sums[1] = sh[1][0];
  }
}

template <int M, int MODE, int LOSS>
int launch_one(const WideArgs& A, int blocks, hipStream_t stream) {
  auto kern = mel_dist_wide_kernel<M, MODE, LOSS>;
  const size_t bytes = (size_t)(fixed_floats<M>(MODE) + row_floats(M, A.n_mels)) * 4;
  if (bytes > (size_t)LDS_CU) return AT_ERR_UNSUPPORTED;
  if (bytes > 64 * 1024) {
    const int e = at::allow_big_lds(reinterpret_cast<const void*>(kern));
    if (e != AT_OK) return e;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(NW * 64), bytes, stream, A);
  AT_LAUNCH_CHECK();
  return AT_OK;
}

template <int M, int LOSS>
int launch_loss(const WideArgs& A, int blocks, hipStream_t stream) {
  if (A.ola.dx) return launch_one<M, DIST_DX, LOSS>(A, blocks, stream);
  return A.G ? launch_one<M, DIST_G, LOSS>(A, blocks, stream) : launch_one<M, DIST_NONE, LOSS>(A, blocks, stream);
}

template <int M>
int launch_wide(const WideArgs& A, int loss, int blocks, hipStream_t stream) {
  return loss == LOSS_L2 ? launch_loss<M, LOSS_L2>(A, blocks, stream) : launch_loss<M, LOSS_L1>(A, blocks, stream);
}

// AT_OK when the kernel takes the shape: every band count up to the cap (at or under n_fft/4 too: the caller routes)
int wide_shape_check(int64_t rows, int64_t T, int n_fft, int hop, int n_mels) {
  if (rows <= 0 || T <= 0 || n_fft <= 0 || hop <= 0 || n_mels <= 0) return AT_ERR_INVALID;
  if (!at_stft_fused_supported(n_fft) || n_fft > 1024 || hop * 4 != n_fft || T <= n_fft / 2) return AT_ERR_UNSUPPORTED;
  if (n_mels > 2 * n_fft || n_mels > MAX_MELS) return AT_ERR_UNSUPPORTED;
  const int64_t n_out = 1 + T / hop;
  if (T >= (1LL << 30) || n_out * (n_fft / 2 + 1) >= (1LL << 31)) return AT_ERR_UNSUPPORTED;   // 32-bit sample / bin indices
  return AT_OK;
}

int64_t wide_max_blocks(int64_t rows, int64_t T, int n_fft, int hop) {
  const int FW = 64 / (n_fft / 32);
  const int64_t gpr = (1 + T / hop + FW - 1) / FW;
  const int64_t blocks = (rows * gpr + NW - 1) / NW;
  return blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS;
}

// resident workgroups of the persistent grid: two per CU (launch bounds) where two band-row sets fit the CU's LDS, else one
int64_t wide_resident(int n_fft, int n_mels, bool dx) {
  return (2 * lds_bytes(n_fft / 2, n_mels, dx) <= LDS_CU ? 2 : 1) * (int64_t)at::device_cu_count();
}

int64_t wide_blocks(int64_t rows, int64_t T, int n_fft, int hop, int n_mels, bool dx) {
  const int64_t blocks = wide_max_blocks(rows, T, n_fft, hop), resident = wide_resident(n_fft, n_mels, dx);
  return blocks < resident ? blocks : resident;
}

// G != null: dL/dX; dx != null: dL/dx through the overlap-add tail (workspace: partials, seam slots, margins)
int wide_run(int loss, const float* x, const float* y, int64_t rows, int64_t T, const float* window, const float* twiddles,
             int n_fft, int hop, const int* bin_bands, const float* bin_w, const int* band_span, int n_mels, float clamp_eps,
             float power, float g_log, float g_mag, float* G, float* dx, double* sums, void* workspace, hipStream_t s) {
  const int M = n_fft / 2, FW = 64 / (M / 16);
  WideArgs A;
  A.x = x; A.y = y; A.window = window; A.tw = reinterpret_cast<const float2*>(twiddles);
  A.bin_bands = bin_bands; A.bin_w = reinterpret_cast<const float2*>(bin_w); A.band_span = band_span;
  A.G = reinterpret_cast<float2*>(G); A.partials = reinterpret_cast<float2*>(workspace);
  A.T = (int)T; A.n_out = (int)(1 + T / hop); A.hop = hop;
  A.gpr = (A.n_out + FW - 1) / FW;
  A.total_groups = rows * A.gpr;
  A.n_mels = n_mels;
  A.eps = clamp_eps;
  A.c_log = (float)((double)power * 0.30102999566398119521);
  // LOSS_L2: d (la - lb)^2 = 2 (la - lb) d la, d (a - b)^2 = 2 (a - b) d a -- the 2 (exact) rides on the weights
  const double two = loss == LOSS_L2 ? 2.0 : 1.0;
  A.g_logp = (float)(two * (double)g_log * (double)power / 2.30258509299404568402);
  A.g_mag = (float)(two * (double)g_mag);
  A.vec2 = ((T % 2) == 0 && (reinterpret_cast<uintptr_t>(x) % 8) == 0 && (reinterpret_cast<uintptr_t>(y) % 8) == 0) ? 1 : 0;
  const int64_t blocks = wide_blocks(rows, T, n_fft, hop, n_mels, dx != nullptr);
  A.ola = OlaOut{};
  if (dx) {
    const int64_t waves = blocks * NW;
    float* ws = reinterpret_cast<float*>(workspace);
    A.ola.dx = dx;
    A.ola.seams = ws + 2 * waves;
    A.ola.margins = A.ola.seams + waves * 3 * hop;
    A.ola.T = (int)T;
    A.ola.Lp = (A.n_out - 1) * hop + n_fft;
    A.ola.n_active = (int)(waves < A.total_groups ? waves : A.total_groups);
  }
  int r = AT_ERR_UNSUPPORTED;
  switch (M) {
    case 16: r = launch_wide<16>(A, loss, (int)blocks, s); break;
    case 32: r = launch_wide<32>(A, loss, (int)blocks, s); break;
    case 64: r = launch_wide<64>(A, loss, (int)blocks, s); break;
    case 128: r = launch_wide<128>(A, loss, (int)blocks, s); break;
    case 256: r = launch_wide<256>(A, loss, (int)blocks, s); break;
    case 512: r = launch_wide<512>(A, loss, (int)blocks, s); break;
  }
  if (r != AT_OK) return r;
  if (dx) {
    OlaFix F;
    F.O = A.ola; F.rows = rows; F.total_groups = A.total_groups; F.gpr = A.gpr; F.FW = FW; F.hop = hop;
    r = ola_fixup(F, s);
    if (r != AT_OK) return r;
  }
  hipLaunchKernelGGL(mel_dist_wide_finalize, dim3(1), dim3(256), 0, s, A.partials, (int)blocks * NW, sums);
  AT_LAUNCH_CHECK();
  return AT_OK;
}

}  // namespace

extern "C" {

int64_t at_mel_dist_wide_workspace_bytes(int64_t rows, int64_t T, int n_fft, int hop, int n_mels) {
  const int e = wide_shape_check(rows, T, n_fft, hop, n_mels);
  if (e != AT_OK) return e;
  return wide_max_blocks(rows, T, n_fft, hop) * NW * (int64_t)sizeof(float2);
}

// the checks and the launch of at_mel_dist_wide_f32 / at_mel_dist_wide_l2_f32
static int wide_entry(int loss, const float* x, const float* y, int64_t rows, int64_t T, const float* window,
                      const float* twiddles, int n_fft, int hop, const int* bin_bands, const float* bin_w, const int* band_span,
                      int n_mels, float clamp_eps, float power, float g_log, float g_mag, float* G, double* sums,
                      void* workspace, int64_t workspace_bytes, void* stream) {
  if (!x || !y || !window || !twiddles || !bin_bands || !bin_w || !band_span || !sums || !workspace) return AT_ERR_INVALID;
  const int e = wide_shape_check(rows, T, n_fft, hop, n_mels);
  if (e != AT_OK) return e;
  if (!(clamp_eps >= FLT_MIN) || !(power > 0.f)) return AT_ERR_UNSUPPORTED;
  if (workspace_bytes < at_mel_dist_wide_workspace_bytes(rows, T, n_fft, hop, n_mels)) return AT_ERR_INVALID;
  return wide_run(loss, x, y, rows, T, window, twiddles, n_fft, hop, bin_bands, bin_w, band_span, n_mels, clamp_eps, power,
                  g_log, g_mag, G, nullptr, sums, workspace, reinterpret_cast<hipStream_t>(stream));
}

int at_mel_dist_wide_f32(const float* x, const float* y, int64_t rows, int64_t T, const float* window, const float* twiddles,
                         int n_fft, int hop, const int* bin_bands, const float* bin_w, const int* band_span, int n_mels,
                         float clamp_eps, float power, float g_log, float g_mag, float* G, double* sums,
                         void* workspace, int64_t workspace_bytes, void* stream) {
  return wide_entry(LOSS_L1, x, y, rows, T, window, twiddles, n_fft, hop, bin_bands, bin_w, band_span, n_mels, clamp_eps, power,
                    g_log, g_mag, G, sums, workspace, workspace_bytes, stream);
}

int at_mel_dist_wide_l2_f32(const float* x, const float* y, int64_t rows, int64_t T, const float* window, const float* twiddles,
                            int n_fft, int hop, const int* bin_bands, const float* bin_w, const int* band_span, int n_mels,
                            float clamp_eps, float power, float g_log, float g_mag, float* G, double* sums,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  return wide_entry(LOSS_L2, x, y, rows, T, window, twiddles, n_fft, hop, bin_bands, bin_w, band_span, n_mels, clamp_eps, power,
                    g_log, g_mag, G, sums, workspace, workspace_bytes, stream);
}

// partials (a float2 per wave), seam slots (3 hops per wave), margins (rows x n_fft)
int64_t at_mel_dist_wide_dx_workspace_bytes(int64_t rows, int64_t T, int n_fft, int hop, int n_mels) {
  const int e = wide_shape_check(rows, T, n_fft, hop, n_mels);
  if (e != AT_OK) return e;
  const int64_t waves = wide_blocks(rows, T, n_fft, hop, n_mels, true) * NW;
  return (waves * (2 + 3 * (int64_t)hop) + rows * n_fft) * (int64_t)sizeof(float);
}

// the checks and the launch of at_mel_dist_wide_dx_f32 / at_mel_dist_wide_dx_l2_f32
static int wide_dx_entry(int loss, const float* x, const float* y, int64_t rows, int64_t T, const float* window,
                         const float* twiddles, int n_fft, int hop, const int* bin_bands, const float* bin_w,
                         const int* band_span, int n_mels, float clamp_eps, float power, float g_log, float g_mag, float* dx,
                         double* sums, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!x || !y || !window || !twiddles || !bin_bands || !bin_w || !band_span || !dx || !sums || !workspace) return AT_ERR_INVALID;
  const int e = wide_shape_check(rows, T, n_fft, hop, n_mels);
  if (e != AT_OK) return e;
  if (!(clamp_eps >= FLT_MIN) || !(power > 0.f)) return AT_ERR_UNSUPPORTED;
  if (workspace_bytes < at_mel_dist_wide_dx_workspace_bytes(rows, T, n_fft, hop, n_mels)) return AT_ERR_INVALID;
  return wide_run(loss, x, y, rows, T, window, twiddles, n_fft, hop, bin_bands, bin_w, band_span, n_mels, clamp_eps, power,
                  g_log, g_mag, nullptr, dx, sums, workspace, reinterpret_cast<hipStream_t>(stream));
}

int at_mel_dist_wide_dx_f32(const float* x, const float* y, int64_t rows, int64_t T, const float* window, const float* twiddles,
                            int n_fft, int hop, const int* bin_bands, const float* bin_w, const int* band_span, int n_mels,
                            float clamp_eps, float power, float g_log, float g_mag, float* dx, double* sums,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  return wide_dx_entry(LOSS_L1, x, y, rows, T, window, twiddles, n_fft, hop, bin_bands, bin_w, band_span, n_mels, clamp_eps,
                       power, g_log, g_mag, dx, sums, workspace, workspace_bytes, stream);
}

int at_mel_dist_wide_dx_l2_f32(const float* x, const float* y, int64_t rows, int64_t T, const float* window, const float* twiddles,
                               int n_fft, int hop, const int* bin_bands, const float* bin_w, const int* band_span, int n_mels,
                               float clamp_eps, float power, float g_log, float g_mag, float* dx, double* sums,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  return wide_dx_entry(LOSS_L2, x, y, rows, T, window, twiddles, n_fft, hop, bin_bands, bin_w, band_span, n_mels, clamp_eps,
                       power, g_log, g_mag, dx, sums, workspace, workspace_bytes, stream);
}

}  // extern "C"
