// Shared device tail of the fused distance kernels (stftdist.hip, meldist.hip) in WAVEFORM mode: from G = dL/dX of a
// frame group, which the kernel has just placed in the wave's slab in bin order, to the overlap-added gradient of the
// SIGNAL.  No spectrum-shaped tensor is written, no torch-side fold follows, no floating-point atomics anywhere.
//
// Per frame (ola_frame): the adjoint of the windowed one-sided DFT with the conventions of ADJ = true in istft.hip,
//     d[n] = window[n] sum_{k=0..M} Re(G[k] e^{+2 pi i k n / n_fft})      (no factor 2 on interior bins, no 1/N)
// the half spectrum is folded into the M-point spectrum of z[n] = d[2n] + i d[2n+1] (DC and Nyquist doubled, the 1/2 on
// the halved window table the kernels already hold), conj(Z) goes through the forward wave FFT of fft_wave.h with the last
// pass in registers, and every lane ends with 32 windowed time samples which it writes, frame after frame, into the wave's
// slab: FW frames x n_fft floats = 2048 floats of the slab's 2176 at every size.
//
// Per group (ola_group): the FW consecutive frames of a group complete exactly FW hop = 512 padded positions.  Lane l owns
// positions l + 64 m (m < 8) and GATHERS each from the at most four frames that cover it, in ascending frame order; what
// frames of earlier groups of the row contributed arrives through a carry of 3 hops (24 L floats).  The carry lives in LDS
// (the kernels are at 242 ... 256 VGPRs), laid out so that element i belongs to lane i % 64 in the gather, in the carry
// update and in the shift FW = 1, 2 need: it is lane-private, no exchange point guards it.  The row's last group also
// emits the 3 hops behind it.  Frame slots past a row's last frame are written as zeros.
//
// Destinations of a padded position p (half = n_fft / 2, Lp = (frames - 1) hop + n_fft; p >= Lp has zero gradient and is
// never written nor read): [half, half + T) -> dx; the two reflected margins -> a (rows, n_fft) workspace.
//
// Seams: a wave's run of groups may begin and end inside a row.  Every wave starts with a zero carry, so what it stores for
// its first 3 hops are partial sums, and its carry at the end of its run holds contributions of ITS frames only: it goes
// to the wave's seam slot.  dist_ola_seams then completes every position behind a boundary exactly once (the latest
// boundary at or in front of a hop owns it and gathers the at most three seams that reach it, oldest first), and
// dist_ola_fold adds the margins onto dx, left then right, one thread per destination.  Both touch rows x n_fft + seam
// elements only; equal inputs give equal bits.
#pragma once
#include "at_common.h"
#include "fft_wave.h"

namespace {

enum DistMode { DIST_NONE = 0, DIST_G = 1, DIST_DX = 2 };   // what a distance kernel produces besides the two sums
enum DistLoss { LOSS_L1 = 0, LOSS_L2 = 1 };                 // how a distance kernel compares: |d| (nn.L1Loss) or d^2 (nn.MSELoss)

struct OlaOut {
  float* dx;         // (rows, T)
  float* seams;      // (waves, 24 L): final carry of every wave whose run ends inside a row
  float* margins;    // (rows, n_fft): padded positions [0, half) and half + T + [0, half)
  int T;
  int Lp;            // padded positions some frame covers
  int n_active;      // waves that own groups (<= groups, so every run is non-empty)
};

template <int M>
constexpr int ola_carry_floats() { return 3 * (M / 2); }

__device__ __forceinline__ void ola_put(const OlaOut& O, int64_t row, int half, int p, float v) {
  if (p >= O.Lp) return;
  if (p < half) O.margins[row * (2 * half) + p] = v;
  else if (p < half + O.T) O.dx[row * O.T + (p - half)] = v;
  else O.margins[row * (2 * half) + (p - O.T)] = v;
}

// G of this lane's frame (fbuf[k], k = 0 .. M, bin order) -> its windowed time frame at slab float fs N + n.
//   s_win: the HALVED window, s_twp: (cos, -sin)(2 pi k / N) for k < M/2, s_tw2 / tw3b: the pass twiddles of the kernels
template <int M>
__device__ __forceinline__ void ola_frame(float2* __restrict__ fbuf, float2* __restrict__ wbuf, const float* __restrict__ s_win,
                                          const float2* __restrict__ s_twp, const float* __restrict__ s_tw2,
                                          const float2* tw3b, int t, int fs, bool valid) {
  using P = Plan<M>;
  constexpr int L = P::L;
  constexpr int NB2 = 16 / P::R2, NB3 = 16 / P::R3;
  float2 a[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int k = t + L * q;
    float2 xk = fbuf[k];
    float2 xm = fbuf[M - k];                            // k == 0: the Nyquist bin
    if (k == 0) { xk = make_float2(2.f * xk.x, 0.f); xm = make_float2(2.f * xm.x, 0.f); }
    const float2 w0 = s_twp[q < 8 ? k : k - M / 2];     // the table holds a quarter turn: k >= M/2 is k - M/2 turned by -i
    const float2 w = q < 8 ? w0 : make_float2(w0.y, -w0.x);
    const float c = w.x, s = -w.y;
    const float sr = xk.x + xm.x, si = xk.y - xm.y;
    const float dr = xk.x - xm.x, di = xk.y + xm.y;
    a[q] = make_float2(sr - s * dr - c * di, -(si + c * dr - s * di));     // conj Z[k]
  }
  wave_sync();
  if constexpr (P::R2 == 1) {
    pass_compute_regs<16, 1, L>(a, nullptr);
  } else {
    pass_compute_store<16, 1, L>(a, fbuf, t, nullptr);
    wave_sync();
    load_points<L>(a, fbuf, t);
    wave_sync();
    float2 tw2[NB2 * P::R2];
#pragma unroll
    for (int b = 0; b < NB2; ++b) {
      const float2* rowp = reinterpret_cast<const float2*>(s_tw2 + ((t + b * L) & 15) * 36);
#pragma unroll
      for (int r = 1; r < P::R2; ++r) tw2[b * P::R2 + r] = rowp[r];
    }
    if constexpr (P::R3 == 1) {
      pass_compute_regs<P::R2, 16, L>(a, tw2);
    } else {
      pass_compute_store<P::R2, 16, L>(a, fbuf, t, tw2);
      wave_sync();
      load_points<L>(a, fbuf, t);
      wave_sync();
      float2 tw3[NB3 * P::R3];
#pragma unroll
      for (int b = 0; b < NB3; ++b) {
        tw3[b * P::R3 + 1] = tw3b[b];
#pragma unroll
        for (int r = 2; r < P::R3; ++r) tw3[b * P::R3 + r] = cmul(tw3[b * P::R3 + r - 1], tw3b[b]);
      }
      pass_compute_regs<P::R3, 16 * P::R2, L>(a, tw3);
    }
  }
  // the slab holds nothing any more: z[n] = conj(Y[n]) w[n], frames packed at stride M
  const float2* w2 = reinterpret_cast<const float2*>(s_win);
  float2* out = wbuf + fs * M;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int n = t + L * q;
    const float2 w = w2[n];
    out[n] = valid ? make_float2(a[q].x * w.x, -a[q].y * w.y) : make_float2(0.f, 0.f);
  }
  wave_sync();
}

// The group's 512 positions (from padded position seg0 hop on) and the new carry; `last`: the row's last group.
template <int M>
__device__ __forceinline__ void ola_group(const float* __restrict__ slab, float* __restrict__ carry, int lane, const OlaOut& O,
                                          int64_t row, int seg0, bool last) {
  using P = Plan<M>;
  constexpr int FW = P::FW, N = 2 * M, HOP = M / 2, CARRY = 3 * HOP, NC = (CARRY + 63) / 64;
  const int p0 = seg0 * HOP;
  // position i of the group: the carry (frames of earlier groups), then frame j - r at its hop r, ascending frames
  auto gather = [&](int i, int j, int o) __attribute__((always_inline)) -> float {
    float acc = i < CARRY ? carry[min(i, CARRY - 1)] : 0.f;
#pragma unroll
    for (int r = 3; r >= 0; --r) {
      const int fr = j - r;
      const float v = slab[max(fr, 0) * N + r * HOP + o];
      acc += fr >= 0 ? v : 0.f;
    }
    return acc;
  };
  if (p0 >= M && p0 + FW * HOP <= M + O.T) {                      // wave-uniform: the whole group lands in dx
    float* __restrict__ drow = O.dx + row * O.T + (p0 - M);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int i = lane + 64 * m;
      if constexpr (HOP >= 64) drow[i] = gather(i, (64 * m) / HOP, lane + (64 * m) % HOP);
      else drow[i] = gather(i, i / HOP, i % HOP);
    }
  } else {                                                        // a group at a row's edge: rolled, one destination at a time
#pragma unroll 1
    for (int m = 0; m < 8; ++m) {
      const int i = lane + 64 * m;
      ola_put(O, row, M, p0 + i, gather(i, i / HOP, i % HOP));
    }
  }
#pragma unroll
  for (int mc = 0; mc < NC; ++mc) {
    const int idx = lane + 64 * mc;
    if (idx < CARRY) {
      const int c = idx / HOP, o = idx % HOP;
      float acc = 0.f;
      if constexpr (FW < 3) {                                     // the old carry reaches past this group: shift it
        if (FW + c < 3) acc = carry[idx + FW * HOP];              // element idx + 512: this lane's, rewritten 8 steps on
      }
#pragma unroll
      for (int r = 3; r >= 1; --r) {
        const int fr = FW + c - r;
        if constexpr (FW >= 3) {
          const float v = slab[min(fr, FW - 1) * N + r * HOP + o];
          acc += fr < FW ? v : 0.f;
        } else {
          if (fr >= 0 && fr < FW) acc += slab[fr * N + r * HOP + o];
        }
      }
      carry[idx] = acc;
    }
  }
  if (last) {                                                     // the 3 hops behind the row's last group; the next row starts at 0
#pragma unroll 1
    for (int idx = lane; idx < CARRY; idx += 64) {
      ola_put(O, row, M, p0 + FW * HOP + idx, carry[idx]);
      carry[idx] = 0.f;
    }
  }
  wave_sync();                                                    // the slab is free again
}

// ---- fix-up kernels: rows x n_fft + seam elements, fixed order, no atomics
struct OlaFix {
  OlaOut O;
  int64_t rows;
  int64_t total_groups;
  int gpr, FW, hop;
};

__device__ __forceinline__ float* ola_dst(const OlaOut& O, int64_t row, int half, int p) {
  if (p < half) return O.margins + row * (2 * half) + p;
  if (p < half + O.T) return O.dx + row * O.T + (p - half);
  return O.margins + row * (2 * half) + (p - O.T);
}

// One workgroup per boundary between the runs of waves w and w + 1.
__global__ __launch_bounds__(256) void dist_ola_seams(const OlaFix F) {
  const int w = blockIdx.x;
  auto bound = [&](int v, int64_t& row, int& seg) -> bool {       // the boundary behind wave v: inside a row?
    const int64_t g = F.total_groups * (v + 1) / F.O.n_active;
    row = g / F.gpr;
    const int gb = (int)(g - row * F.gpr);
    seg = gb * F.FW;
    return gb != 0;
  };
  int64_t row, row1 = -1;
  int e, e1 = 0;
  if (!bound(w, row, e)) return;
  const bool nxt = w + 2 < F.O.n_active && bound(w + 1, row1, e1) && row1 == row;
  const int half = 2 * F.hop;
  for (int idx = threadIdx.x; idx < 3 * F.hop; idx += 256) {
    const int c = idx / F.hop, o = idx - c * F.hop;
    const int s = e + c;
    if (nxt && e1 <= s) continue;                                 // a later boundary owns this hop
    const int p = s * F.hop + o;
    if (p >= F.O.Lp) continue;
    float acc = 0.f;
    for (int v = max(w - 2, 0); v <= w; ++v) {                    // oldest first; runs are non-empty: at most these three reach s
      int64_t rv;
      int ev;
      if (!bound(v, rv, ev) || rv != row || s - ev > 2) continue;
      acc += F.O.seams[(int64_t)v * (3 * F.hop) + (s - ev) * F.hop + o];
    }
    float* d = ola_dst(F.O, row, half, p);
    *d = acc + *d;
  }
}

// One thread per destination of a margin: dx[i] = (dx[i] + left) + right.
__global__ __launch_bounds__(256) void dist_ola_fold(const OlaFix F) {
  const int half = 2 * F.hop, N = 2 * half, T = F.O.T;
  const int64_t total = F.rows * N;
  for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id < total; id += (int64_t)gridDim.x * 256) {
    const int64_t row = id / N;
    const int u = (int)(id - row * N);
    const float* __restrict__ mg = F.O.margins + row * N;
    float* __restrict__ d = F.O.dx + row * T;
    if (u < half) {
      const int i = 1 + u;                                        // padded position half - i mirrors x[i]
      float v = d[i] + mg[half - i];
      const int j = T - 2 - i;                                    // padded position half + T + j mirrors x[T - 2 - j]
      if (j >= 0 && j < half && half + T + j < F.O.Lp) v += mg[half + j];
      d[i] = v;
    } else {
      const int j = N - 1 - u;
      const int i = T - 2 - j;
      if ((i >= 1 && i <= half) || half + T + j >= F.O.Lp) continue;   // the left thread of i has added it / no frame covers it
      d[i] += mg[half + j];
    }
  }
}

// seams, then margins (stream order)
inline int ola_fixup(const OlaFix& F, hipStream_t stream) {
  if (F.O.n_active > 1) {
    hipLaunchKernelGGL(dist_ola_seams, dim3((unsigned)(F.O.n_active - 1)), dim3(256), 0, stream, F);
    AT_LAUNCH_CHECK();
  }
  const int64_t total = F.rows * 4 * F.hop;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(dist_ola_fold, dim3((unsigned)blocks), dim3(256), 0, stream, F);
  AT_LAUNCH_CHECK();
  return AT_OK;
}

}  // namespace
