// Fused SI-SDR loss (reference audiotools/metrics/distance.py:43-131): two streaming kernels and a tiny one.
//
//   sisdr_sums_kernel    grid (S, rows): both signals read ONCE; per workgroup five float64 partial sums
//                        (sum ref, sum est, sum ref^2, sum est^2, sum ref est) of one segment of one item
//   sisdr_finish_kernel  one wave per item: partials -> sums -> loss and the six coefficients of the gradient
//   sisdr_grad_kernel    grid (S, rows): d loss_b / d est = go_b (a est + b ref + c), likewise for ref, both from one read
//
// The loss of an item is a function of its five sums; with the means and alpha folded in algebraically (centred sums
// Crr = Srr - Sr^2/N ..., residual energy Cee - 2 alpha Cre + alpha^2 Crr) one pass over the signals is enough.  That
// expansion cancels: it is evaluated on float64 sums of exact products (a float32 times a float32 is exact in double), which
// keeps it within 4e-8 dB of the explicit formulation up to 60 dB SDR.  The gradient with respect to either signal is affine in
// the two signals per item, so backward needs no saved intermediate: six floats per item.  No temporary is written, no atomics:
// equal inputs give equal bits on one device.  DESIGN.md 5.13.
#include "at_common.h"

namespace {

constexpr int NT = 256;                 // lanes of a workgroup (four waves)
constexpr int DEPTH = 4;                // 16-byte loads in flight per lane and signal
constexpr int TILE = NT * 4 * DEPTH;    // 4096 floats of each signal per workgroup iteration
constexpr int MAX_ROWS = 65535;         // gridDim.y

struct Quad { float v[4]; };

// Four consecutive floats; `vec` (wave-uniform) = the address is 16-byte aligned.
__device__ __forceinline__ Quad load4(const float* __restrict__ p, bool vec) {
  Quad q;
  if (vec) {
    const float4 u = *reinterpret_cast<const float4*>(p);
    q.v[0] = u.x; q.v[1] = u.y; q.v[2] = u.z; q.v[3] = u.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) q.v[k] = p[k];
  }
  return q;
}
// the ragged end of an item: elements at or past `left` read as 0 (they add nothing to any sum)
__device__ __forceinline__ Quad load4_guard(const float* __restrict__ p, int64_t left) {
  Quad q;
#pragma unroll
  for (int k = 0; k < 4; ++k) q.v[k] = k < left ? p[k] : 0.0f;
  return q;
}
// non-temporal: the gradient is read next by another kernel's first touch at the earliest
__device__ __forceinline__ void store4(float* __restrict__ p, const Quad& q, bool vec) {
  if (vec) {
    const at::v4f_t u = {q.v[0], q.v[1], q.v[2], q.v[3]};
    __builtin_nontemporal_store(u, reinterpret_cast<at::v4f_t*>(p));
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) __builtin_nontemporal_store(q.v[k], p + k);
  }
}
__device__ __forceinline__ void store4_guard(float* __restrict__ p, const Quad& q, int64_t left) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < left) __builtin_nontemporal_store(q.v[k], p + k);
}
__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct Acc {
  double r = 0.0, e = 0.0, rr = 0.0, ee = 0.0, re = 0.0;
  __device__ __forceinline__ void add(const Quad& qr, const Quad& qe) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double x = (double)qr.v[k], y = (double)qe.v[k];
      r += x;
      e += y;
      rr = fma(x, x, rr);
      ee = fma(y, y, ee);
      re = fma(x, y, re);
    }
  }
};

// Workgroup (s, b): elements [s seg, min(N, (s + 1) seg)) of item b, seg a multiple of TILE.  Lane t of iteration i holds
// elements i TILE + (j NT + t) 4 ... + 3, j < DEPTH: every load instruction of a wave covers 1 KB of consecutive memory.
__global__ __launch_bounds__(NT) void sisdr_sums_kernel(const float* __restrict__ ref, const float* __restrict__ est, int64_t N,
                                                        int64_t seg, double* __restrict__ partials) {
  const int64_t b = blockIdx.y;
  const float* __restrict__ pr = ref + b * N;
  const float* __restrict__ pe = est + b * N;
  const bool vr = aligned16(pr), ve = aligned16(pe);     // seg and every lane offset are multiples of 16 bytes
  const int64_t lo = (int64_t)blockIdx.x * seg;
  const int64_t hi = lo + seg < N ? lo + seg : N;
  const int t = threadIdx.x;
  Acc acc;
  int64_t i = lo;
  for (; i + TILE <= hi; i += TILE) {
    Quad qr[DEPTH], qe[DEPTH];
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) qr[j] = load4(pr + i + (j * NT + t) * 4, vr);
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) qe[j] = load4(pe + i + (j * NT + t) * 4, ve);
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) acc.add(qr[j], qe[j]);
  }
  if (i < hi) {
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) {
      const int64_t at = i + (j * NT + t) * 4;
      if (at < hi) acc.add(load4_guard(pr + at, hi - at), load4_guard(pe + at, hi - at));
    }
  }
  // wave tree, then the four waves in ascending order
  __shared__ double sh[NT / 64][5];
  const double w[5] = {at::wave_sum(acc.r), at::wave_sum(acc.e), at::wave_sum(acc.rr), at::wave_sum(acc.ee),
                       at::wave_sum(acc.re)};
  if ((t & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) sh[t >> 6][k] = w[k];
  }
  __syncthreads();
  if (t < 5) {
    double s = sh[0][t];
#pragma unroll
    for (int v = 1; v < NT / 64; ++v) s += sh[v][t];
    partials[(b * gridDim.x + blockIdx.x) * 5 + t] = s;
  }
}

// One wave per item.  Lane l adds partials l, l + 64, ... in ascending order, then the wave tree; lane 0 does the rest in
// double.  With x = est, y = ref centred, Cee = sum x^2, Cre = sum x y, Crr = sum y^2:
//   alpha = (Cre + eps) / (Crr + eps) | 1,   St = alpha^2 Crr,   Sres = Cee - 2 alpha Cre + St,   loss = -10 log10(St / Sres + eps)
//   d loss = p dSt + q dSres,   p = k / Sres,  q = -k St / Sres^2,  k = -10 / (ln 10 (St / Sres + eps))
//          = q dCee + (u - 2 alpha q) dCre + ((p + q) alpha^2 - u alpha) dCrr,   u = 2 (alpha Crr (p + q) - Cre q) / (Crr + eps) | 0
// dCee/dest = 2 x, dCre/dest = y, dCre/dref = x, dCrr/dref = 2 y; centring maps a x + b y to a est + b ref - (a mean_est + b mean_ref).
__global__ __launch_bounds__(64) void sisdr_finish_kernel(const double* __restrict__ partials, int S, int64_t N, int scaling,
                                                          int zero_mean, int has_clip, float clip_min,
                                                          float* __restrict__ loss, float* __restrict__ coef,
                                                          double* __restrict__ sums) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = lane; i < S; i += 64) {
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k] += partials[(b * S + i) * 5 + k];
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) s[k] = at::wave_sum(s[k]);
  if (lane != 0) return;
#pragma unroll
  for (int k = 0; k < 5; ++k) sums[b * 5 + k] = s[k];
  const double eps = 1e-8;
  double mr = 0.0, me = 0.0, Crr = s[2], Cee = s[3], Cre = s[4];
  if (zero_mean) {
    mr = s[0] / (double)N;
    me = s[1] / (double)N;
    Crr -= s[0] * mr;
    Cee -= s[1] * me;
    Cre -= s[0] * me;
  }
  const double D = Crr + eps;
  const double alpha = scaling ? (Cre + eps) / D : 1.0;
  const double St = alpha * alpha * Crr;
  const double Sres = Cee - 2.0 * alpha * Cre + St;
  const double ratio = St / Sres;
  double L = -10.0 * log10(ratio + eps);
  const double k = -4.3429448190325182765 / (ratio + eps);      // -10 / ln 10
  const double p = k / Sres, q = -k * St / (Sres * Sres);
  const double u = scaling ? 2.0 * (alpha * Crr * (p + q) - Cre * q) / D : 0.0;
  const double cre = u - 2.0 * alpha * q, crr = (p + q) * alpha * alpha - u * alpha;
  double c[6] = {2.0 * q, cre, 0.0, cre, 2.0 * crr, 0.0};
  c[2] = -(c[0] * me + c[1] * mr);
  c[5] = -(c[3] * me + c[4] * mr);
  if (has_clip && L < (double)clip_min) {        // torch.clamp: the value of the bound, no gradient below it
    L = (double)clip_min;
#pragma unroll
    for (int j = 0; j < 6; ++j) c[j] = 0.0;
  }
  loss[b] = (float)L;
#pragma unroll
  for (int j = 0; j < 6; ++j) coef[b * 6 + j] = (float)c[j];
}

// One output value: go (a est + b ref + c) evaluated in double (float32 coefficient times float32 go is exact) and rounded once.
__device__ __forceinline__ Quad affine(const Quad& qe, const Quad& qr, double a, double b, double c) {
  Quad o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o.v[k] = (float)fma(a, (double)qe.v[k], fma(b, (double)qr.v[k], c));
  return o;
}

template <bool WANT_EST, bool WANT_REF>
__global__ __launch_bounds__(NT) void sisdr_grad_kernel(const float* __restrict__ ref, const float* __restrict__ est, int64_t N,
                                                        int64_t seg, const float* __restrict__ coef,
                                                        const float* __restrict__ go, float* __restrict__ d_ref,
                                                        float* __restrict__ d_est) {
  const int64_t b = blockIdx.y;
  const float* __restrict__ pr = ref + b * N;
  const float* __restrict__ pe = est + b * N;
  float* __restrict__ oe = WANT_EST ? d_est + b * N : nullptr;
  float* __restrict__ orf = WANT_REF ? d_ref + b * N : nullptr;
  const bool vr = aligned16(pr), ve = aligned16(pe), voe = aligned16(oe), vor = aligned16(orf);
  const double g = (double)go[b];
  double ce[3], cr[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ce[k] = g * (double)coef[b * 6 + k];
    cr[k] = g * (double)coef[b * 6 + 3 + k];
  }
  const int64_t lo = (int64_t)blockIdx.x * seg;
  const int64_t hi = lo + seg < N ? lo + seg : N;
  const int t = threadIdx.x;
  int64_t i = lo;
  for (; i + TILE <= hi; i += TILE) {
    Quad qr[DEPTH], qe[DEPTH];
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) qr[j] = load4(pr + i + (j * NT + t) * 4, vr);
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) qe[j] = load4(pe + i + (j * NT + t) * 4, ve);
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) {
      const int64_t at = i + (j * NT + t) * 4;
      if constexpr (WANT_EST) store4(oe + at, affine(qe[j], qr[j], ce[0], ce[1], ce[2]), voe);
      if constexpr (WANT_REF) store4(orf + at, affine(qe[j], qr[j], cr[0], cr[1], cr[2]), vor);
    }
  }
  if (i < hi) {
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) {
      const int64_t at = i + (j * NT + t) * 4;
      if (at < hi) {
        const Quad qr = load4_guard(pr + at, hi - at), qe = load4_guard(pe + at, hi - at);
        if constexpr (WANT_EST) store4_guard(oe + at, affine(qe, qr, ce[0], ce[1], ce[2]), hi - at);
        if constexpr (WANT_REF) store4_guard(orf + at, affine(qe, qr, cr[0], cr[1], cr[2]), hi - at);
      }
    }
  }
}

// Segments per item: rows * S workgroups fill the device about eight times over (up to eight workgroups of 256 lanes are
// resident per CU), a segment is a whole number of tiles, and S never exceeds the tiles of an item.
struct Split { int S; int64_t seg; };
Split split_item(int64_t rows, int64_t N) {
  const int64_t tiles = (N + TILE - 1) / TILE;
  const int64_t want = (8 * (int64_t)at::device_cu_count() + rows - 1) / rows;
  const int64_t per = (tiles + want - 1) / want;            // tiles per segment, >= 1
  return Split{(int)((tiles + per - 1) / per), per * TILE};
}

int shape_check(int64_t rows, int64_t N) {
  if (rows <= 0 || N <= 0) return AT_ERR_INVALID;
  if (rows > MAX_ROWS || N >= (1LL << 31)) return AT_ERR_UNSUPPORTED;
  return AT_OK;
}

}  // namespace

extern "C" {

int64_t at_sisdr_workspace_bytes(int64_t rows, int64_t N) {
  const int e = shape_check(rows, N);
  if (e != AT_OK) return e;
  return rows * split_item(rows, N).S * 5 * (int64_t)sizeof(double);
}

int at_sisdr_f32(const float* ref, const float* est, int64_t rows, int64_t N, int scaling, int zero_mean, int has_clip,
                 float clip_min, float* loss, float* coef, double* sums, void* workspace, int64_t workspace_bytes,
                 void* stream) {
  if (!ref || !est || !loss || !coef || !sums || !workspace) return AT_ERR_INVALID;
  const int e = shape_check(rows, N);
  if (e != AT_OK) return e;
  if (workspace_bytes < at_sisdr_workspace_bytes(rows, N)) return AT_ERR_INVALID;
  const Split sp = split_item(rows, N);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* partials = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(sisdr_sums_kernel, dim3((unsigned)sp.S, (unsigned)rows), dim3(NT), 0, s, ref, est, N, sp.seg, partials);
  AT_LAUNCH_CHECK();
  hipLaunchKernelGGL(sisdr_finish_kernel, dim3((unsigned)rows), dim3(64), 0, s, partials, sp.S, N, scaling, zero_mean,
                     has_clip, clip_min, loss, coef, sums);
  AT_LAUNCH_CHECK();
  return AT_OK;
}

int at_sisdr_grad_f32(const float* ref, const float* est, int64_t rows, int64_t N, const float* coef, const float* go,
                      float* d_ref, float* d_est, void* stream) {
  if (!ref || !est || !coef || !go || (!d_ref && !d_est)) return AT_ERR_INVALID;
  const int e = shape_check(rows, N);
  if (e != AT_OK) return e;
  const Split sp = split_item(rows, N);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)sp.S, (unsigned)rows);
  if (d_ref && d_est)
    hipLaunchKernelGGL((sisdr_grad_kernel<true, true>), grid, dim3(NT), 0, s, ref, est, N, sp.seg, coef, go, d_ref, d_est);
  else if (d_est)
    hipLaunchKernelGGL((sisdr_grad_kernel<true, false>), grid, dim3(NT), 0, s, ref, est, N, sp.seg, coef, go, d_ref, d_est);
  else
    hipLaunchKernelGGL((sisdr_grad_kernel<false, true>), grid, dim3(NT), 0, s, ref, est, N, sp.seg, coef, go, d_ref, d_est);
  AT_LAUNCH_CHECK();
  return AT_OK;
}

}  // extern "C"
