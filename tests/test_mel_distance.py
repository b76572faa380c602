"""The fused mel-spectrogram distance (csrc/meldist.hip, kernels.mel_distance, MelSpectrogramLoss(fused=True)) against a
float64 torch formulation of the same formulas.  Inputs: those of tests/test_stft_distance.py."""
import math

import numpy as np
import pytest
import torch

import audiotools_amd as A
from audiotools_amd import _native, kernels, metrics, tables
from tests import synth

EPS, SR = 1e-5, 44100


def _inputs(T, device="cpu"):
    """(3, 2, T) estimate and target: item 1 shares a stretch of digital silence, item 2 is silent in x only."""
    x = synth.audio_batch(3, 2, T, seed=3, gaps=False)
    y = synth.audio_batch(3, 2, T, seed=4, gaps=False)
    lo, hi = T // 5, T - T // 8
    x[1:, :, lo:hi] = 0
    y[1, :, lo:hi] = 0
    return x.to(device), y.to(device)


def _formulation(x, y, n_fft, n_mels, p, dtype):
    """X, the dense basis, a = mel_x, b = mel_y (rows, n_mels, N) and the two log terms in ``dtype``."""
    win = A.AudioSignal.get_window("hann", n_fft, str(x.device)).to(dtype)
    X, Y = (torch.stft(s.to(dtype).flatten(0, 1), n_fft, n_fft // 4, window=win, center=True, return_complex=True) for s in (x, y))
    basis = torch.from_numpy(tables.mel_filters_np(SR, n_fft, n_mels, 0.0, None)).to(x.device, dtype)
    a, b = basis @ X.abs(), basis @ Y.abs()
    return X, basis, a, b, p * torch.log10(a.clamp(EPS)), p * torch.log10(b.clamp(EPS))


def _sums_and_grad(x, y, n_fft, n_mels, p, g_log, g_mag, dtype):
    X, basis, a, b, la, lb = _formulation(x, y, n_fft, n_mels, p, dtype)
    gmel = g_mag * torch.sign(a - b) + g_log * torch.sign(a.clamp(EPS) - b.clamp(EPS)) * (a >= EPS) * p / (math.log(10) * a.clamp(EPS))
    mag = X.abs()
    G = torch.where(mag > 0, (basis.T @ gmel) / mag * X, torch.zeros_like(X))
    return torch.stack([(la - lb).abs().sum(), (a - b).abs().sum()]), G, a, b, basis, mag


def _kernel(x, y, n_fft, n_mels, p, g_log, g_mag, want_grad=True):
    win = A.AudioSignal.get_window("hann", n_fft, "cuda:0")
    tb = tables.mel_dist_tables(SR, n_fft, n_mels, 0.0, None, x.device)
    return kernels.mel_distance(x, y, win, n_fft, n_fft // 4, tb, n_mels, EPS, p, g_log, g_mag, want_grad)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1100, 4100])
@pytest.mark.parametrize("n_fft,n_mels", [(32, 5), (64, 16), (512, 80), (1024, 160), (2048, 320), (2048, 150)])
def test_kernel_vs_float64(n_fft, n_mels, T):
    """sums within 1e-4; G, away from the sign-ambiguous bins, no further from float64 than twice the float32 torch
    formulation.  Measured per case (kernel, float32 torch): profiles/r08_notes.md."""
    p, lw, mw = {(512, 1100): (1.0, 0.5, 1.0), (1024, 4100): (1.0, 1.0, 0.0), (2048, 4100): (1.0, 1.0, 0.0)}.get((n_fft, T), (2.0, 1.0, 1.0))
    x, y = _inputs(T, "cuda")
    count = 6 * (1 + T // (n_fft // 4)) * n_mels
    g_log, g_mag = lw / count, mw / count
    sums, G = _kernel(x, y, n_fft, n_mels, p, g_log, g_mag)
    s64, G64, a, b, basis, mag = _sums_and_grad(x, y, n_fft, n_mels, p, g_log, g_mag, torch.float64)
    G32 = _sums_and_grad(x, y, n_fft, n_mels, p, g_log, g_mag, torch.float32)[1]
    G = G.reshape(G64.shape)
    assert G.dtype == torch.complex64 and G.stride(-2) == 1, "bin-contiguous: what stft_adjoint reads without a copy"
    top = torch.maximum(a, b)
    amb_band = (top > 0) & (((a - b).abs() <= 1e-4 * top) | ((a - EPS).abs() <= 1e-4 * EPS) | ((b - EPS).abs() <= 1e-4 * EPS))
    amb = ((basis != 0).double().T @ amb_band.double()) > 0        # a bin is ambiguous when a band that weighs on it is
    scale = G64.abs().max()
    err = float(((G - G64).abs() * ~amb).max() / scale)
    err32 = float(((G32 - G64).abs() * ~amb).max() / scale)
    silent = mag == 0
    print(f"n_fft={n_fft} n_mels={n_mels} T={T}: sums rel {((sums - s64).abs() / s64).tolist()}, G err {err:.3e} "
          f"(float32 torch {err32:.3e}), excluded {float(amb.float().mean()):.2e}, silent bins {int(silent.sum())}")
    assert torch.all((sums - s64).abs() <= 1e-4 * s64)
    assert float(amb.float().mean()) <= 0.01
    assert bool(torch.isfinite(torch.view_as_real(G)).all()) and bool((G[silent] == 0).all())
    assert err <= 2 * err32 + 1e-5


@pytest.mark.gpu
def test_public_path_fused_vs_unfused():
    x, y = _inputs(4100)
    mels, scales = [5, 10, 80, 320], [32, 64, 512, 2048]
    x64 = x.double().requires_grad_(True)
    v64 = 0.0
    for n, w in zip(mels, scales):
        _, _, _, _, la, lb = _formulation(x64, y, w, n, 1.0, torch.float64)
        v64 = v64 + (la - lb).abs().mean()
    (g64,) = torch.autograd.grad(v64, x64)

    def run(fused, est_first, n_mels=mels, lengths=scales):
        xa, yc = x.clone().cuda().requires_grad_(True), y.clone().cuda()
        sx, sy = A.AudioSignal(xa, SR), A.AudioSignal(yc, SR)
        k = len(lengths)
        loss = metrics.spectral.MelSpectrogramLoss(n_mels=n_mels, window_lengths=lengths, mel_fmin=[0] * k, mel_fmax=[None] * k,
                                                   pow=1.0, mag_weight=0.0, fused=fused)
        val = loss(sx, sy) if est_first else loss(sy, sx)
        (g,) = torch.autograd.grad(val, xa)
        return float(val), g.cpu(), (sx.stft_data, sy.stft_data)

    for est_first in (True, False):
        v1, g1, data = run(True, est_first)
        v0, g0, _ = run(False, est_first)
        e1, e0 = (float((g - g64).abs().max() / g64.abs().max()) for g in (g1, g0))
        print(f"est_first={est_first}: value fused {v1} unfused {v0} float64 {float(v64)}; gradient err fused {e1:.3e} unfused {e0:.3e}")
        assert abs(v1 - v0) <= 1e-4 * abs(v0)
        assert data == (None, None), "the fused path leaves stft_data alone"
        assert e1 <= 2 * e0 + 1e-5
    v1, v0 = (run(f, True, [320, 80], [2048, 400])[0] for f in (True, False))      # 400: not a kernel size, runs as before
    assert abs(v1 - v0) <= 1e-4 * abs(v0)


@pytest.mark.gpu
def test_bit_equal_on_every_run():
    x, y = _inputs(4100, "cuda")
    (s1, G1), (s2, G2) = (_kernel(x, y, 512, 80, 2.0, 1e-3, 1e-3) for _ in range(2))
    s3, G3 = _kernel(x, y, 512, 80, 2.0, 1e-3, 1e-3, want_grad=False)
    assert torch.equal(s1, s2) and torch.equal(s1, s3) and G3 is None
    assert torch.equal(torch.view_as_real(G1.contiguous()), torch.view_as_real(G2.contiguous()))


def test_fused_on_cpu_is_the_unfused_code():
    x, y = _inputs(1100)

    def run(fused):
        xa = x.clone().requires_grad_(True)
        loss = metrics.spectral.MelSpectrogramLoss(n_mels=[80, 10], window_lengths=[512, 64], fused=fused)
        val = loss(A.AudioSignal(xa, SR), A.AudioSignal(y.clone(), SR))
        return val.detach(), torch.autograd.grad(val, xa)[0]

    (v1, g1), (v0, g0) = run(True), run(False)
    assert torch.equal(v1, v0) and torch.equal(g1, g0)


def test_argument_validation_without_gpu():
    _native.build()
    lib = _native.lib()
    p = _native.ptr(torch.zeros(4096))

    def call(x=p, n_fft=512, hop=128, n_mels=80, spans=p, sums=p, eps=EPS, T=4096):
        return lib.at_mel_dist_f32(x, p, 1, T, p, p, n_fft, hop, p, p, spans, n_mels, eps, 2.0, 1.0, 1.0, None, sums, p, 1 << 20, None)

    assert call(x=None) == -1 and call(sums=None) == -1 and call(spans=None) == -1
    assert call(n_mels=129) == -2 and call(hop=100) == -2 and call(n_fft=4096, hop=1024) == -2 and call(T=256) == -2
    assert call(eps=1e-40) == -2
    assert lib.at_mel_dist_workspace_bytes(0, 4096, 512, 128, 80) == -1
    assert lib.at_mel_dist_workspace_bytes(1, 4096, 512, 128, 129) == -2 and lib.at_mel_dist_workspace_bytes(1, 4096, 512, 100, 80) == -2
    assert lib.at_mel_dist_workspace_bytes(6, 4096, 512, 128, 80) > 0


@pytest.mark.parametrize("n_fft,n_mels", [(32, 5), (64, 16), (2048, 320)])
def test_band_spans_with_bin_table_give_the_dense_basis(n_fft, n_mels):
    basis = tables.mel_filters_np(SR, n_fft, n_mels, 0.0, None)
    (bands, w), spans = tables.mel_bin_table_np(basis), tables.mel_band_spans_np(basis)
    dense = np.zeros_like(basis)
    for m, sp in enumerate(spans):
        for k in range(sp & 0xffff, (sp & 0xffff) + (sp >> 16)):
            dense[m, k] = w[k, 0] if (bands[k] & 0xffff) == m else w[k, 1]
    assert np.array_equal(dense, basis) and np.array_equal(dense.sum(1), basis.sum(1))
    assert n_fft != 64 or int((spans >> 16 == 0).sum()) == 2       # (64, 16): two all-zero bands
    gap = basis.copy()
    gap[-1, np.nonzero(gap[-1])[0][1]] = 0                          # a hole in the last band: no span form
    assert n_fft < 2048 or tables.mel_band_spans_np(gap) is None
