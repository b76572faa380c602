"""Fused SI-SDR kernels (csrc/wavedist.hip) and ``SISDRLoss(fused=True)`` against the formulation of ``SISDRLoss.forward``
evaluated in float64 on the same float32 inputs."""
import functools

import pytest
import torch

from audiotools_amd import AudioSignal, kernels
from audiotools_amd.metrics.distance import SISDRLoss
from tests import synth

# (B, C, T, est is a view one element into a larger buffer): less than one wave; two segments and odd N (items 1.. misaligned);
# ten segments with a ragged tail; fully aligned; a storage offset of 4 bytes
CASES = {"37": (4, 1, 37, False), "2x4099": (4, 2, 4099, False), "40003": (4, 1, 40003, False),
         "2x32768": (4, 2, 32768, False), "view": (4, 1, 8192, True)}
WEIGHTS = (1.0, 0.3, 2.5, 0.7)      # upstream gradient of the un-reduced loss


@functools.lru_cache(maxsize=None)
def _inputs(B, C, T):
    """ref: item 1 carries a DC offset of 0.5, the last item is silent; est = 0.7 ref + noise at 0, 30, 60 dB SDR."""
    ref = synth.audio_batch(B, C, T, seed=5)
    ref[1] += 0.5
    ref[-1] = 0
    noise = torch.randn(B, C, T, generator=torch.Generator().manual_seed(6))
    est = 0.7 * ref
    for b, db in enumerate((0, 30, 60)):
        est[b] += noise[b] * ((0.7 * ref[b]).norm() / noise[b].norm() * 10 ** (-db / 20))
    est[-1] = 0.01 * noise[-1]
    return ref, est


def _on_gpu(case):
    B, C, T, view = CASES[case]
    ref, est = _inputs(B, C, T)
    r = ref.cuda()
    if not view:
        return r, est.cuda()
    e = torch.empty(est.numel() + 1, device="cuda")[1:].view(B, C, T)
    return r, e.copy_(est)


@functools.lru_cache(maxsize=None)
def _reference(case, scaling, zero_mean, clip_min, reduction):
    """float64: the per-item loss (B, 1) and the gradients of the reduced loss with respect to ref and est."""
    B, C, T, _ = CASES[case]
    ref, est = (t.double().requires_grad_(True) for t in _inputs(B, C, T))
    loss = SISDRLoss(scaling, "none", zero_mean, clip_min)(ref, est)
    _reduce(loss, reduction).backward()
    return loss.detach(), ref.grad, est.grad


def _reduce(loss, reduction):
    if reduction == "none":
        return (loss * torch.tensor(WEIGHTS, dtype=loss.dtype, device=loss.device)[:, None]).sum()
    return loss.mean() if reduction == "mean" else loss.sum()


@pytest.mark.gpu
@pytest.mark.parametrize("clip_min", [None, -30])
@pytest.mark.parametrize("zero_mean", [True, False])
@pytest.mark.parametrize("scaling", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_value(case, scaling, zero_mean, clip_min):
    """|loss - loss64| <= 2e-5 dB: the one-pass expansion on float64 sums stays within 4e-8 dB of the explicit float64
    formulation at these SDRs and offsets (CPU emulation), the float32 result below 128 in magnitude adds 3.8e-6 dB; 5 x margin."""
    r, e = _on_gpu(case)
    loss, coef, sums = kernels.sisdr(r, e, scaling, zero_mean, clip_min)
    want = _reference(case, scaling, zero_mean, clip_min, "sum")[0]
    err = (loss.cpu().double() - want).abs()
    print(f"{case}: loss error {err.flatten().tolist()} dB")
    assert loss.shape == (r.shape[0], 1) and float(err[:-1].max()) <= 2e-5
    assert float(loss[-1]) == 80.0                     # silent ref: Srr = 0 exactly
    r64, e64 = r.cpu().double().flatten(1), e.cpu().double().flatten(1)
    s64 = torch.stack([r64.sum(1), e64.sum(1), (r64 * r64).sum(1), (e64 * e64).sum(1), (r64 * e64).sum(1)], 1)
    rel = (sums.cpu() - s64).abs() / s64.abs().clamp_min(1e-300)
    print(f"{case}: sums relative error {float(rel.max()):.2e}")
    assert float(rel.max()) <= 1e-12
    again = kernels.sisdr(r, e, scaling, zero_mean, clip_min)
    assert all(torch.equal(a, b) for a, b in zip((loss, coef, sums), again))


@pytest.mark.gpu
@pytest.mark.parametrize("wrt", ["est", "ref", "both"])
@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
@pytest.mark.parametrize("scaling,zero_mean,clip_min", [(True, True, -30), (True, False, None), (False, True, None),
                                                        (False, False, -30)])
@pytest.mark.parametrize("case", CASES)
def test_gradient(case, scaling, zero_mean, clip_min, reduction, wrt):
    """Against float64 autograd.  The per-item coefficients of g64 = a est + b ref + c come from a least-squares fit whose
    residual must vanish (the gradient is affine); then |g - g64| <= 2**-22 (|a est| + |b ref| + |c|) element-wise: each term
    carries one float32 coefficient rounding and at most one operation rounding of 2**-24 -- derived, not measured.  An item
    under the clamp has g64 = 0, hence a zero bound: its gradient is exactly zero."""
    r, e = _on_gpu(case)
    r.requires_grad_(wrt != "est")
    e.requires_grad_(wrt != "ref")
    _reduce(SISDRLoss(scaling, "none", zero_mean, clip_min, fused=True)(r, e), reduction).backward()
    _, gr64, ge64 = _reference(case, scaling, zero_mean, clip_min, reduction)
    r64, e64 = r.detach().cpu().double().flatten(1), e.detach().cpu().double().flatten(1)
    assert (r.grad is None) == (wrt == "est") and (e.grad is None) == (wrt == "ref")
    for name, g, g64 in (("ref", r.grad, gr64), ("est", e.grad, ge64)):
        if g is None:
            continue
        g, g64 = g.cpu().double().flatten(1), g64.flatten(1)
        for b in range(g.shape[0]):
            A = torch.stack([e64[b], r64[b], torch.ones_like(r64[b])], 1)
            abc = torch.linalg.lstsq(A, g64[b][:, None]).solution
            scale = (A.abs() @ abc.abs())[:, 0]
            assert float(((A @ abc)[:, 0] - g64[b]).abs().max()) <= 1e-9 * float(scale.max()), "float64 gradient not affine"
            err, bound = (g[b] - g64[b]).abs(), 2.0 ** -22 * scale
            worst = int((err - bound).argmax())
            print(f"{case} d{name}[{b}]: error {float(err[worst]):.3e} where the bound is {float(bound[worst]):.3e}")
            assert bool((err <= bound).all())


@pytest.mark.gpu
@pytest.mark.parametrize("wrt", ["x", "y", "both"])
def test_public_path(wrt):
    r, e = _on_gpu("2x4099")
    r.requires_grad_(wrt != "y")
    e.requires_grad_(wrt != "x")
    loss = SISDRLoss(reduction="none", fused=True)(AudioSignal(r, 44100), AudioSignal(e, 44100))
    assert loss.grad_fn.name() == "_FusedSISDRBackward"
    assert torch.equal(loss.detach(), kernels.sisdr(r.detach(), e.detach())[0])
    assert float((loss.detach().cpu().double() - _reference("2x4099", True, True, None, "sum")[0]).abs()[:-1].max()) <= 2e-5
    loss.mean().backward()
    for t, wanted in ((r, wrt != "y"), (e, wrt != "x")):
        assert (t.grad is not None) == wanted and (not wanted or bool(torch.isfinite(t.grad).all()))


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_cpu_inputs_run_the_unfused_code(reduction):
    ref, est = _inputs(4, 2, 4099)
    ref, est = ref[:3], est[:3]
    assert SISDRLoss().fused is False
    want = SISDRLoss(reduction=reduction, clip_min=-30)(ref, est)
    assert torch.equal(SISDRLoss(reduction=reduction, clip_min=-30, fused=True)(ref, est), want)
    assert torch.equal(SISDRLoss(reduction=reduction, clip_min=-30, fused=True)(AudioSignal(ref, 44100), AudioSignal(est, 44100)), want)
