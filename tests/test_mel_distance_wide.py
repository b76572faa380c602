"""The fused mel distance for filterbanks with more than window / 4 bands (csrc/meldist_wide.hip; kernels.mel_distance and
mel_distance_dx route there) against the float64 torch formulation on the CPU, G and dx from float64 autograd.  Inputs and
formulation: tests/test_mel_distance.py.  Bounds: sums within 1e-4; a gradient error may be twice that of the same
formulation in float32 torch plus the floor the mel kernels already have (1e-5 for L1, 4.7e-5 for L2).  G excludes the bins
under a band whose sign (L1) or clamp (L2) float32 rounding may flip, as tests/test_mel_distance.py and
tests/test_distance_mse.py do; dx of L1 excludes nothing (tests/test_distance_waveform_grad.py).  Measured figures per
case: profiles/r12_notes.md."""
import functools

import pytest
import torch

import audiotools_amd as A
from audiotools_amd import _native, kernels, metrics, tables
from tests.test_mel_distance import EPS, SR, _formulation, _inputs

P, LW, MW = 2.0, 0.7, 1.3
FLOOR = {"l1": 1e-5, "l2": 4.7e-5}
SIZES = [(32, 9), (32, 64), (64, 64), (256, 80), (512, 129), (1024, 512), (1024, 257)]


@functools.lru_cache(maxsize=None)
def _reference(n_fft, n_mels, T, norm, dtype):
    """sums, G = dL/dX and dx = dL/dx of L = (LW sums[0] + MW sums[1]) / count in ``dtype``; the bins and samples excluded."""
    x, y = _inputs(T)
    xd = x.to(dtype).requires_grad_(True)
    X, basis, a, b, la, lb = _formulation(xd, y, n_fft, n_mels, P, dtype)
    dist = (lambda u, v: (u - v).abs().sum()) if norm == "l1" else (lambda u, v: ((u - v) ** 2).sum())
    sums = torch.stack([dist(la, lb), dist(a, b)])
    G, dx = torch.autograd.grad((LW * sums[0] + MW * sums[1]) / a.numel(), [X, xd])
    a, b = a.detach(), b.detach()
    if norm == "l1":
        top = torch.maximum(a, b)
        amb = (top > 0) & (((a - b).abs() <= 1e-4 * top) | ((a - EPS).abs() <= 1e-4 * EPS) | ((b - EPS).abs() <= 1e-4 * EPS))
    else:
        amb = (a - EPS).abs() <= 1e-3 * EPS
    amb_G = ((basis != 0).to(torch.float64).T @ amb.to(torch.float64)) > 0
    amb_dx = torch.zeros(x.shape, dtype=torch.bool)
    if norm == "l2":       # the samples under a frame with such a band (one reflection), as tests/test_distance_mse.py
        pad = torch.nn.functional.conv_transpose1d(amb.to(torch.float64).amax(1, keepdim=True),
                                                   torch.ones(1, 1, n_fft, dtype=torch.float64), stride=n_fft // 4)[:, 0]
        idx = (torch.arange(pad.shape[1]) - n_fft // 2).abs()
        amb_dx = (torch.zeros(pad.shape[0], T, dtype=torch.float64).index_add_(1, torch.where(idx >= T, 2 * (T - 1) - idx, idx), pad) > 0).reshape(x.shape)
    return dict(sums=sums.detach(), G=G, dx=dx, amb_G=amb_G, amb_dx=amb_dx, count=a.numel(), silent=X.detach().abs() == 0)


def _kernel(x, y, n_fft, n_mels, norm, mode, g_log, g_mag):
    win = A.AudioSignal.get_window("hann", n_fft, "cuda:0")
    args = (x, y, win, n_fft, n_fft // 4, tables.mel_dist_tables(SR, n_fft, n_mels, 0.0, None, x.device), n_mels, EPS, P, g_log, g_mag)
    return kernels.mel_distance_dx(*args, loss=norm) if mode == "dx" else kernels.mel_distance(*args, True, loss=norm)


@pytest.mark.gpu
@pytest.mark.parametrize("short,norm,mode", [(False, "l1", "G"), (False, "l2", "dx"), (True, "l2", "G"), (True, "l1", "dx")])
@pytest.mark.parametrize("n_fft,n_mels", SIZES)
def test_kernel_vs_float64(n_fft, n_mels, short, norm, mode):
    """T = 1100 (ragged) and T = n_fft/2 + 1 (both margins fold over the whole row): every size meets both norms, both
    gradient modes and both lengths."""
    T = n_fft // 2 + 1 if short else 1100
    r64, r32 = (_reference(n_fft, n_mels, T, norm, d) for d in (torch.float64, torch.float32))
    x, y = (s.cuda() for s in _inputs(T))
    sums, grad = _kernel(x, y, n_fft, n_mels, norm, mode, LW / r64["count"], MW / r64["count"])
    ref, amb, cap = r64[mode], r64["amb_" + mode], {"G": 0.01, "dx": 0.05}[mode]
    got = grad.cpu().reshape(ref.shape)
    err, err32 = (float(((g.to(ref.dtype) - ref).abs() * ~amb).max() / ref.abs().max()) for g in (got, r32[mode]))
    rel = (sums.cpu() - r64["sums"]).abs() / r64["sums"]
    print(f"n_fft={n_fft} n_mels={n_mels} T={T} {norm} {mode}: sums rel {rel.tolist()}, err {err:.3e} (float32 torch {err32:.3e}), "
          f"excluded {float(amb.double().mean()):.2e}")
    assert bool((rel <= 1e-4).all())
    assert float(amb.double().mean()) <= cap
    assert bool(torch.isfinite(torch.view_as_real(got) if mode == "G" else got).all())
    if mode == "G":
        assert grad.dtype == torch.complex64 and grad.stride(-2) == 1, "bin-contiguous: what stft_adjoint reads without a copy"
        assert bool((got[r64["silent"]] == 0).all()), "digital silence: exactly zero"
    assert err32 <= 2e-3, "the float32 reference is too noisy to set a bound"
    assert err <= 2 * err32 + FLOOR[norm]


@pytest.mark.gpu
@pytest.mark.parametrize("est_first", [True, False])
@pytest.mark.parametrize("fused", [True, "waveform"])
def test_public_path_64_bands_at_every_scale(fused, est_first):
    scales, T = [32, 64, 128, 256, 512, 1024], 4100
    x, y = _inputs(T)
    x64 = x.double().requires_grad_(True)
    v64 = 0.0
    for w in scales:
        _, _, a, b, la, lb = _formulation(x64, y, w, 64, P, torch.float64)
        v64 = v64 + (la - lb).abs().mean() + (a - b).abs().mean()
    (g64,) = torch.autograd.grad(v64, x64)

    def run(fused):
        xa, yc = x.clone().cuda().requires_grad_(True), y.clone().cuda()
        sx, sy = A.AudioSignal(xa, SR), A.AudioSignal(yc, SR)
        loss = metrics.spectral.MelSpectrogramLoss(n_mels=[64] * 6, window_lengths=scales, mel_fmin=[0] * 6, mel_fmax=[None] * 6, fused=fused)
        val = loss(sx, sy) if est_first else loss(sy, sx)
        (g,) = torch.autograd.grad(val, xa)
        return float(val.detach()), float((g.cpu() - g64).abs().max() / g64.abs().max()), (sx.stft_data, sy.stft_data)

    (v1, e1, data), (v0, e0, _) = run(fused), run(False)
    print(f"fused={fused} est_first={est_first}: value {v1} unfused {v0} float64 {float(v64)}; gradient err {e1:.3e} unfused {e0:.3e}")
    assert abs(v1 - v0) <= 1e-4 * abs(v0)
    assert e1 <= 2 * e0 + 1e-5
    assert data == (None, None), "every scale ran fused: stft_data is untouched"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["G", "dx"])
def test_bit_equal_on_every_run(mode):
    x, y = (s.cuda() for s in _inputs(1100))
    (s1, g1), (s2, g2) = (_kernel(x, y, 256, 80, "l1", mode, 1e-3, 1e-3) for _ in range(2))
    assert torch.equal(s1, s2) and torch.equal(torch.view_as_real(g1.contiguous()) if mode == "G" else g1, torch.view_as_real(g2.contiguous()) if mode == "G" else g2)


@pytest.mark.parametrize("name", ["at_mel_dist_wide_f32", "at_mel_dist_wide_l2_f32", "at_mel_dist_wide_dx_f32", "at_mel_dist_wide_dx_l2_f32"])
def test_argument_validation_without_gpu(name):
    _native.build()
    lib = _native.lib()
    p = _native.ptr(torch.zeros(4096))

    def call(x=p, n_fft=256, hop=64, n_mels=80, spans=p, out=p, sums=p, eps=EPS, T=4096):
        return getattr(lib, name)(x, p, 1, T, p, p, n_fft, hop, p, p, spans, n_mels, eps, 2.0, 1.0, 1.0, out, sums, p, 1 << 24, None)

    assert call(x=None) == -1 and call(sums=None) == -1 and call(spans=None) == -1 and call(T=0) == -1
    assert "_dx" not in name or call(out=None) == -1
    assert call(n_mels=513) == -2 and call(n_fft=64, hop=16, n_mels=129) == -2 and call(hop=100) == -2
    assert call(n_fft=4096, hop=1024) == -2 and call(n_fft=2048, hop=512) == -2 and call(T=128) == -2 and call(eps=1e-40) == -2
    nbytes = lib.at_mel_dist_wide_dx_workspace_bytes if "_dx" in name else lib.at_mel_dist_wide_workspace_bytes
    assert nbytes(0, 4096, 256, 64, 80) == -1 and nbytes(1, 4096, 256, 64, 513) == -2 and nbytes(1, 4096, 256, 100, 80) == -2
    assert nbytes(6, 4096, 256, 64, 80) > 0 and nbytes(6, 4096, 256, 64, 512) > 0
    for supported in (kernels.mel_distance_supported, kernels.mel_distance_dx_supported):
        assert supported(256, 64, 1100, 80, 1e-5, 2.0) and supported(32, 8, 1100, 64, 1e-5, 2.0) and supported(2048, 512, 1100, 512, 1e-5, 2.0)
        assert not supported(256, 64, 1100, 513, 1e-5, 2.0) and not supported(64, 16, 1100, 129, 1e-5, 2.0)
