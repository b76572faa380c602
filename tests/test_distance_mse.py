"""The squared-error (nn.MSELoss) variant of the fused STFT / mel distance kernels (csrc/stftdist.hip, csrc/meldist.hip,
``loss="l2"``) against the float64 torch formulation on the CPU, gradients from float64 autograd.

Bounds: an error may be twice that of the SAME formulation evaluated in float32 torch, plus a floor for the cases where
float32 torch happens to land within an ulp.  The floors are twice the largest kernel error measured over all cases of
this file, per kernel (profiles/r11_notes.md, section 2): sums 2.84e-7 (stft) and 7.10e-7 (mel), G / dx 3.54e-4 (stft) and
2.35e-5 (mel).  The gradient errors of the STFT distance are those of the few bins with |X| just above the clamp, where
1 / |X| amplifies the rounding of the transform; float32 torch has the same ones (1.0e-5 ... 3.2e-4 on the same cases)."""
import functools

import pytest
import torch
from torch import nn

import audiotools_amd as A
from audiotools_amd import kernels, metrics, tables
from tests import synth

EPS, SR, P = 1e-5, 44100, 2.0
SUM_FLOOR = {"stft": 5.7e-7, "mel": 1.42e-6}      # relative, on a sum
GRAD_FLOOR = {"stft": 7.1e-4, "mel": 4.7e-5}      # on max|error| / max|reference| of G or dx
SIZES = [("stft", n, 0) for n in (32, 64, 512, 2048)] + [("mel", n, n // 8) for n in (32, 64, 512, 2048)] + [("mel", 64, 16)]


def _inputs(T):
    """tests/test_stft_distance.py::_inputs: item 1 shares a stretch of digital silence, item 2 is silent in x only."""
    x = synth.audio_batch(3, 2, T, seed=3, gaps=False)
    y = synth.audio_batch(3, 2, T, seed=4, gaps=False)
    lo, hi = T // 5, T - T // 8
    x[1:, :, lo:hi] = 0
    y[1, :, lo:hi] = 0
    return x, y


@functools.lru_cache(maxsize=None)
def _reference(kind, n_fft, n_mels, T, lw, mw, swap, dtype):
    """The formulation in ``dtype`` on the CPU with nn.MSELoss(reduction="sum") semantics, weights lw / count and mw / count:
    sums, value, G = dL/dX, dx = dL/d estimate (``swap``: the estimate is y), and the masks of the clamp-ambiguous elements."""
    est, ref = _inputs(T)[::-1] if swap else _inputs(T)
    est, hop = est.to(dtype).requires_grad_(True), n_fft // 4
    win = A.AudioSignal.get_window("hann", n_fft, "cpu").to(dtype)
    X, Y = (torch.stft(s.to(dtype).flatten(0, 1), n_fft, hop, window=win, center=True, return_complex=True) for s in (est, ref))
    a, b, spread = X.abs(), Y.abs(), None
    if kind == "mel":
        basis = torch.from_numpy(tables.mel_filters_np(SR, n_fft, n_mels, 0.0, None)).to(dtype)
        a, b, spread = basis @ a, basis @ b, (basis != 0).double().T
    mse = nn.MSELoss(reduction="sum")
    sums = torch.stack([mse(P * a.clamp(EPS).log10(), P * b.clamp(EPS).log10()), mse(a, b)])
    value = (lw * sums[0] + mw * sums[1]) / a.numel()
    G, dx = torch.autograd.grad(value, [X, est])
    amb = ((a.detach() - EPS).abs() <= 1e-3 * EPS).double()             # [a >= eps] may flip under float32 rounding
    amb_G = (amb if spread is None else spread @ amb) > 0               # mel: the bins a band weighs on
    pad = torch.nn.functional.conv_transpose1d(amb.amax(1, keepdim=True), torch.ones(1, 1, n_fft, dtype=torch.float64), stride=hop)[:, 0]
    idx = (torch.arange(pad.shape[1]) - n_fft // 2).abs()               # padded position -> sample (one reflection)
    amb_dx = torch.zeros(pad.shape[0], T, dtype=torch.float64).index_add_(1, torch.where(idx >= T, 2 * (T - 1) - idx, idx), pad) > 0
    return dict(sums=sums.detach(), value=value.detach(), G=G, dx=dx.flatten(0, 1), amb_G=amb_G, amb_dx=amb_dx, count=a.numel())


def _check_grad(kind, got, key, r64, r32, cap):
    ref, amb = r64[key], r64["amb_" + key]
    err, err32 = (float(((g.to(ref.dtype) - ref).abs() * ~amb).max() / ref.abs().max()) for g in (got, r32[key]))
    print(f"  {key}: err {err:.3e} float32 torch {err32:.3e} excluded {float(amb.double().mean()):.2e}")
    assert float(amb.double().mean()) <= cap
    assert bool(torch.isfinite(got).all()) and bool((got[ref == 0] == 0).all()), "digital silence: exactly zero"
    assert err <= 2 * err32 + GRAD_FLOOR[kind]


def _kernel(kind, mode, x, y, n_fft, n_mels, g_log, g_mag):
    win = A.AudioSignal.get_window("hann", n_fft, "cuda:0")
    args = (x, y, win, n_fft, n_fft // 4) + ((tables.mel_dist_tables(SR, n_fft, n_mels, 0.0, None, x.device), n_mels) if kind == "mel" else ())
    fn = getattr(kernels, kind + ("_distance_dx" if mode == "dx" else "_distance"))
    return fn(*args, EPS, P, g_log, g_mag, *(() if mode == "dx" else (mode == "G",)), loss="l2")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sums", "G", "dx"])
@pytest.mark.parametrize("T", [1100, 4100])
@pytest.mark.parametrize("kind,n_fft,n_mels", SIZES)
def test_kernel_vs_float64(kind, n_fft, n_mels, T, mode):
    r64, r32 = (_reference(kind, n_fft, n_mels, T, 0.7, 1.3, False, d) for d in (torch.float64, torch.float32))
    x, y = (s.cuda() for s in _inputs(T))
    sums, grad = _kernel(kind, mode, x, y, n_fft, n_mels, 0.7 / r64["count"], 1.3 / r64["count"])
    rel, rel32 = (((s.cpu().double() - r64["sums"]).abs() / r64["sums"]) for s in (sums, r32["sums"]))
    print(f"{kind} n_fft={n_fft} n_mels={n_mels} T={T} {mode}: sums rel {rel.tolist()} float32 torch {rel32.tolist()}")
    assert bool((rel <= 2 * rel32 + SUM_FLOOR[kind]).all())
    if mode == "G":
        assert grad.dtype == torch.complex64 and grad.stride(-2) == 1, "bin-contiguous: what stft_adjoint reads without a copy"
        _check_grad(kind, grad.cpu().reshape(r64["G"].shape), "G", r64, r32, 1e-3)
    if mode == "dx":
        _check_grad(kind, grad.cpu().flatten(0, 1), "dx", r64, r32, 0.05)
    assert mode != "sums" or grad is None


@pytest.mark.gpu
@pytest.mark.parametrize("wrt_y", [False, True])
@pytest.mark.parametrize("fused", [True, "waveform"])
@pytest.mark.parametrize("kind", ["stft", "mel"])
def test_public_path(kind, fused, wrt_y):
    T, scales, mels = 4100, [2048, 512, 64], [256, 64, 8]
    parts = [[_reference(kind, w, m if kind == "mel" else 0, T, 1.0, 1.0, wrt_y, d) for w, m in zip(scales, mels)]
             for d in (torch.float64, torch.float32)]
    r64, r32 = ({"value": sum(r["value"] for r in rs), "dx": sum(r["dx"] for r in rs),
                 "amb_dx": functools.reduce(torch.logical_or, [r["amb_dx"] for r in rs])} for rs in parts)
    xa, ya = (s.cuda().requires_grad_(g) for s, g in zip(_inputs(T), (not wrt_y, wrt_y)))
    x, y, leaf = A.AudioSignal(xa, SR), A.AudioSignal(ya, SR), ya if wrt_y else xa
    if kind == "stft":
        loss = metrics.spectral.MultiScaleSTFTLoss(window_lengths=scales, loss_fn=nn.MSELoss(), fused=fused)
    else:
        loss = metrics.spectral.MelSpectrogramLoss(n_mels=mels, window_lengths=scales, mel_fmin=[0.0] * 3, mel_fmax=[None] * 3,
                                                   loss_fn=nn.MSELoss(), fused=fused)
    val = loss(x, y)
    todo, names = [val.grad_fn], set()
    while todo:
        node = todo.pop()
        names.add(node.name())
        todo += [n for n, _ in node.next_functions if n is not None]
    want = {"stft": "_StftDistance", "mel": "_MelDistance"}[kind] + ("Wave" if fused == "waveform" else "") + "Backward"
    assert names - {"AddBackward0", "torch::autograd::AccumulateGrad"} == {want}, names
    (g,) = torch.autograd.grad(val, leaf)
    rel, rel32 = (abs(float(v) - float(r64["value"])) / float(r64["value"]) for v in (val.detach(), r32["value"]))
    print(f"{kind} fused={fused} wrt_y={wrt_y}: value rel {rel:.3e} float32 torch {rel32:.3e}")
    assert rel <= 2 * rel32 + SUM_FLOOR[kind]
    _check_grad(kind, g.cpu().flatten(0, 1), "dx", r64, r32, 0.05)
    assert x.stft_data is None and y.stft_data is None, "the fused path leaves stft_data alone"


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n_mels", [("stft", 0), ("mel", 64)])
def test_bit_equal_on_every_run(kind, n_mels):
    x, y = (s.cuda() for s in _inputs(4100))
    (s1, d1), (s2, d2) = (_kernel(kind, "dx", x, y, 512, n_mels, 1e-3, 1e-3) for _ in range(2))
    assert torch.equal(s1, s2) and torch.equal(d1, d2)


def test_cpu_tensors_unknown_norm_and_sum_reduction():
    x, y = _inputs(1100)

    def run(cls, fused, loss_fn):
        xa = x.clone().requires_grad_(True)
        kw = dict(n_mels=[64, 8]) if cls is metrics.spectral.MelSpectrogramLoss else {}
        val = cls(window_lengths=[512, 64], loss_fn=loss_fn, fused=fused, **kw)(A.AudioSignal(xa, SR), A.AudioSignal(y.clone(), SR))
        return val.detach(), torch.autograd.grad(val, xa)[0]

    for cls in (metrics.spectral.MultiScaleSTFTLoss, metrics.spectral.MelSpectrogramLoss):
        for loss_fn in (nn.MSELoss(), nn.MSELoss(reduction="sum")):
            (v1, g1), (v0, g0) = run(cls, True, loss_fn), run(cls, False, loss_fn)
            assert torch.equal(v1, v0) and torch.equal(g1, g0)
    win = torch.hann_window(512)
    for call in (lambda: kernels.stft_distance(x, y, win, 512, 128, EPS, P, 1.0, 1.0, True, loss="l3"),
                 lambda: kernels.stft_distance_dx(x, y, win, 512, 128, EPS, P, 1.0, 1.0, loss="l3"),
                 lambda: kernels.mel_distance(x, y, win, 512, 128, None, 64, EPS, P, 1.0, 1.0, True, loss="l3"),
                 lambda: kernels.mel_distance_dx(x, y, win, 512, 128, None, 64, EPS, P, 1.0, 1.0, loss="l3"),
                 lambda: kernels.stft_distance_supported(512, 128, 1100, EPS, P, loss="l3"),
                 lambda: kernels.mel_distance_dx_supported(512, 128, 1100, 64, EPS, P, loss="l3")):
        with pytest.raises(ValueError):          # CPU tensors and no tables: raised before anything native is touched
            call()
