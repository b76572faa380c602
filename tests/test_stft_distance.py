"""The fused STFT-magnitude distance (csrc/stftdist.hip, kernels.stft_distance, MultiScaleSTFTLoss(fused=True)) against a
float64 torch formulation of the same formulas."""
import math

import pytest
import torch
from torch import nn

import audiotools_amd as A
from audiotools_amd import _native, kernels, metrics
from tests import synth

EPS = 1e-5


def _inputs(T, device="cpu"):
    """(3, 2, T) estimate and target: item 1 shares a stretch of digital silence (a = b = 0), item 2 is silent in x only."""
    x = synth.audio_batch(3, 2, T, seed=3, gaps=False)
    y = synth.audio_batch(3, 2, T, seed=4, gaps=False)
    lo, hi = T // 5, T - T // 8
    x[1:, :, lo:hi] = 0
    y[1, :, lo:hi] = 0
    return x.to(device), y.to(device)


def _formulation(x, y, n_fft, p, dtype):
    """X, a = |X|, b = |Y| and the two log terms in ``dtype`` (the package's float32 window, torch.stft, (rows, F, N))."""
    win = A.AudioSignal.get_window("hann", n_fft, str(x.device)).to(dtype)
    X, Y = (torch.stft(s.to(dtype).flatten(0, 1), n_fft, n_fft // 4, window=win, center=True, return_complex=True) for s in (x, y))
    a, b = X.abs(), Y.abs()
    return X, a, b, p * torch.log10(a.clamp(EPS)), p * torch.log10(b.clamp(EPS))


def _sums_and_grad(x, y, n_fft, p, g_log, g_mag, dtype):
    X, a, b, la, lb = _formulation(x, y, n_fft, p, dtype)
    coef = g_mag * torch.sign(a - b) + g_log * torch.sign(a.clamp(EPS) - b.clamp(EPS)) * (a >= EPS) * p / (math.log(10) * a)
    G = torch.where(a > 0, coef / a * X, torch.zeros_like(X))
    return torch.stack([(la - lb).abs().sum(), (a - b).abs().sum()]), G, a, b


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1100, 4100])
@pytest.mark.parametrize("n_fft", [32, 64, 512, 1024, 2048])
def test_kernel_vs_float64(n_fft, T):
    """sums within 1e-4; G, away from the sign-ambiguous elements, no further from float64 than twice the float32 torch
    formulation.  Measured max|dG| / max|G| per case (kernel, float32 torch): profiles/r07_notes.md."""
    p, lw, mw = {(512, 1100): (1.0, 0.5, 1.0), (1024, 4100): (2.0, 1.0, 0.0)}.get((n_fft, T), (2.0, 1.0, 1.0))
    x, y = _inputs(T, "cuda")
    count = 6 * (1 + T // (n_fft // 4)) * (n_fft // 2 + 1)
    g_log, g_mag = lw / count, mw / count
    win = A.AudioSignal.get_window("hann", n_fft, "cuda:0")
    sums, G = kernels.stft_distance(x, y, win, n_fft, n_fft // 4, EPS, p, g_log, g_mag, True)
    s64, G64, a, b = _sums_and_grad(x, y, n_fft, p, g_log, g_mag, torch.float64)
    _, G32, _, _ = _sums_and_grad(x, y, n_fft, p, g_log, g_mag, torch.float32)
    G = G.reshape(G64.shape)
    assert G.dtype == torch.complex64 and G.stride(-2) == 1, "bin-contiguous: what stft_adjoint reads without a copy"
    top = torch.maximum(a, b)
    amb = (top > 0) & (((a - b).abs() <= 1e-4 * top) | ((a - EPS).abs() <= 1e-4 * EPS) | ((b - EPS).abs() <= 1e-4 * EPS))
    scale = G64.abs().max()
    err = float(((G - G64).abs() * ~amb).max() / scale)
    err32 = float(((G32 - G64).abs() * ~amb).max() / scale)
    silent = (a == 0) & (b == 0)
    print(f"n_fft={n_fft} T={T}: sums rel {((sums - s64).abs() / s64).tolist()}, G err {err:.3e} (float32 torch {err32:.3e}), "
          f"excluded {float(amb.float().mean()):.2e}, shared-silence bins {int(silent.sum())}")
    assert torch.all((sums - s64).abs() <= 1e-4 * s64)
    assert float(amb.float().mean()) <= 0.01
    assert bool(torch.isfinite(torch.view_as_real(G)).all()) and bool((G[silent] == 0).all())
    assert n_fft > 512 or int(silent.sum()) > 0       # (the short windows fit whole frames into the silence)
    assert err <= 2 * err32 + 1e-5


@pytest.mark.gpu
def test_public_path_fused_vs_unfused():
    x, y = _inputs(4100)
    scales = [2048, 512, 64]
    x64 = x.double().requires_grad_(True)
    v64 = 0.0
    for w in scales:
        _, a, b, la, lb = _formulation(x64, y, w, 2.0, torch.float64)
        v64 = v64 + (la - lb).abs().mean() + (a - b).abs().mean()
    (g64,) = torch.autograd.grad(v64, x64)

    def run(fused, est_first, lengths=scales):
        xa, yc = x.clone().cuda().requires_grad_(True), y.clone().cuda()
        sx, sy = A.AudioSignal(xa, 44100), A.AudioSignal(yc, 44100)
        loss = metrics.spectral.MultiScaleSTFTLoss(window_lengths=lengths, fused=fused)
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
    v1, v0 = run(True, True, [2048, 400])[0], run(False, True, [2048, 400])[0]      # 400: not a fused size, runs as before
    assert abs(v1 - v0) <= 1e-4 * abs(v0)


@pytest.mark.gpu
def test_bit_equal_on_every_run():
    x, y = _inputs(4100, "cuda")
    win = A.AudioSignal.get_window("hann", 512, "cuda:0")
    s1, G1 = kernels.stft_distance(x, y, win, 512, 128, EPS, 2.0, 1e-3, 1e-3, True)
    s2, G2 = kernels.stft_distance(x, y, win, 512, 128, EPS, 2.0, 1e-3, 1e-3, True)
    s3, G3 = kernels.stft_distance(x, y, win, 512, 128, EPS, 2.0, 1e-3, 1e-3, False)
    assert torch.equal(s1, s2) and torch.equal(s1, s3) and G3 is None
    assert torch.equal(torch.view_as_real(G1.contiguous()), torch.view_as_real(G2.contiguous()))


def test_fused_on_cpu_is_the_unfused_code():
    x, y = _inputs(1100)

    def run(fused):
        xa = x.clone().requires_grad_(True)
        val = metrics.spectral.MultiScaleSTFTLoss(window_lengths=[512, 64], fused=fused)(A.AudioSignal(xa, 44100), A.AudioSignal(y.clone(), 44100))
        return val.detach(), torch.autograd.grad(val, xa)[0]

    (v1, g1), (v0, g0) = run(True), run(False)
    assert torch.equal(v1, v0) and torch.equal(g1, g0)


def test_argument_validation_without_gpu():
    _native.build()
    lib = _native.lib()
    buf = torch.zeros(4096)
    p = _native.ptr(buf)

    def call(x=p, n_fft=512, hop=128, sums=p, eps=EPS, T=4096):
        return lib.at_stft_dist_f32(x, p, 1, T, p, p, n_fft, hop, eps, 2.0, 1.0, 1.0, None, sums, p, 1 << 20, None)

    assert call(x=None) == -1 and call(sums=None) == -1
    assert call(n_fft=4096, hop=1024) == -2 and call(hop=100) == -2 and call(T=256) == -2 and call(eps=1e-20) == -2
    assert lib.at_stft_dist_workspace_bytes(0, 4096, 512, 128) == -1
    assert lib.at_stft_dist_workspace_bytes(1, 4096, 4096, 1024) == -2 and lib.at_stft_dist_workspace_bytes(1, 4096, 512, 100) == -2
    assert lib.at_stft_dist_workspace_bytes(6, 4096, 512, 128) > 0
