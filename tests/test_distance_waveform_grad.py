"""The waveform mode of the fused distances (csrc/dist_ola.h; kernels.stft_distance_dx / mel_distance_dx; fused="waveform"):
loss sums and dL/dx from one kernel, against float64 torch.  Inputs and formulations: those of tests/test_stft_distance.py and
tests/test_mel_distance.py.  Measured figures per case: profiles/r09_notes.md."""
import pytest
import torch

import audiotools_amd as A
from audiotools_amd import _native, kernels, metrics, tables
from tests.test_mel_distance import _formulation as _mel_formulation
from tests.test_stft_distance import _formulation as _stft_formulation
from tests.test_stft_distance import _inputs

EPS, SR = 1e-5, 44100
KINDS = ["stft", "mel"]
F32_EPS = float(torch.finfo(torch.float32).eps)


def _n_mels(n_fft):
    return min(n_fft // 4, 320)


def _reference(kind, x, y, n_fft, p, lw, mw, dtype):
    """(sums, count, dL/dx) of L = lw mean|log difference| + mw mean|difference| in ``dtype``, by autograd."""
    xd = x.to(dtype).requires_grad_(True)
    if kind == "stft":
        _, a, b, la, lb = _stft_formulation(xd, y, n_fft, p, dtype)
    else:
        _, _, a, b, la, lb = _mel_formulation(xd, y, n_fft, _n_mels(n_fft), p, dtype)
    sums = torch.stack([(la - lb).abs().sum(), (a - b).abs().sum()])
    (g,) = torch.autograd.grad(sums[0] * (lw / a.numel()) + sums[1] * (mw / a.numel()), xd)
    return sums.detach(), a.numel(), g


def _kernel(kind, x, y, n_fft, p, g_log, g_mag, mode):
    """mode "dx": (sums, dx) of the waveform kernel; "G": (sums, G) of the existing kernel."""
    win = A.AudioSignal.get_window("hann", n_fft, "cuda:0")
    args = (x, y, win, n_fft, n_fft // 4)
    if kind == "mel":
        args += (tables.mel_dist_tables(SR, n_fft, _n_mels(n_fft), 0.0, None, x.device), _n_mels(n_fft))
    args += (EPS, p, g_log, g_mag)
    fn = {"stft": (kernels.stft_distance, kernels.stft_distance_dx), "mel": (kernels.mel_distance, kernels.mel_distance_dx)}[kind]
    return fn[1](*args) if mode == "dx" else fn[0](*args, True)


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft,T", [(32, 1100), (64, 4101), (512, 257), (512, 1100), (1024, 4100), (2048, 1025), (2048, 4100),
                                     (32, 700001), (256, 700001), (2048, 700001)])
@pytest.mark.parametrize("kind", KINDS)
def test_dx_vs_float64_autograd(kind, n_fft, T):
    """sums within 1e-4 of float64; dx no further from float64 autograd than twice the float32 torch formulation + 1e-5."""
    x, y = _inputs(T, "cuda")
    for p, lw, mw in ((2.0, 1.0, 1.0), (1.0, 1.0, 0.0)):
        s64, count, g64 = _reference(kind, x, y, n_fft, p, lw, mw, torch.float64)
        g32 = _reference(kind, x, y, n_fft, p, lw, mw, torch.float32)[2]
        sums, dx = _kernel(kind, x, y, n_fft, p, lw / count, mw / count, "dx")
        assert dx.shape == x.shape and dx.dtype == torch.float32
        scale = g64.abs().max()
        err = float((dx - g64).abs().max() / scale)
        err32 = float((g32 - g64).abs().max() / scale)
        print(f"{kind} n_fft={n_fft} T={T} pow={p} mag_weight={mw}: sums rel {((sums - s64).abs() / s64.clamp(1e-300)).tolist()}, "
              f"dx err {err:.3e} (float32 torch {err32:.3e})")
        assert torch.all((sums - s64).abs() <= 1e-4 * s64)
        assert err32 <= 2e-3, "the float32 reference is too noisy to set a bound"
        assert err <= 2 * err32 + 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft,T", [(32, 1100), (512, 257), (1024, 4100), (2048, 4100), (256, 700001)])
@pytest.mark.parametrize("kind", KINDS)
def test_dx_vs_float64_adjoint_of_the_same_G(kind, n_fft, T):
    """The in-kernel tail against kernels.stft_adjoint on the G of the existing kernel, both measured against the float64
    linear adjoint of that G.  Floor: the rounding of a four-term sum and a store."""
    x, y = _inputs(T, "cuda")
    count = 6 * (1 + T // (n_fft // 4)) * (n_fft // 2 + 1 if kind == "stft" else _n_mels(n_fft))
    sums_g, G = _kernel(kind, x, y, n_fft, 2.0, 1.0 / count, 1.0 / count, "G")
    sums, dx = _kernel(kind, x, y, n_fft, 2.0, 1.0 / count, 1.0 / count, "dx")
    win = A.AudioSignal.get_window("hann", n_fft, "cuda:0")
    xd = x.double().requires_grad_(True)
    X = torch.stft(xd.flatten(0, 1), n_fft, n_fft // 4, window=win.double(), center=True, return_complex=True)
    Gd = G.flatten(0, 1).to(torch.complex128)
    (ref,) = torch.autograd.grad((Gd.real * X.real + Gd.imag * X.imag).sum(), xd)
    e_old = float((kernels.stft_adjoint(G, win, n_fft, n_fft // 4, T) - ref).abs().max())
    e_new = float((dx - ref).abs().max())
    print(f"{kind} n_fft={n_fft} T={T}: e_old {e_old:.3e} e_new {e_new:.3e} max|ref| {float(ref.abs().max()):.3e}")
    assert torch.equal(sums, sums_g)
    assert e_new <= 2 * e_old + 4 * F32_EPS * float(ref.abs().max())


def _public_loss(kind, fused, lengths=None):
    if kind == "stft":
        return metrics.spectral.MultiScaleSTFTLoss(window_lengths=lengths or [2048, 512, 64], fused=fused)
    lengths = lengths or [32, 64, 512, 2048]
    mels = [{32: 5, 64: 10, 512: 80, 2048: 320, 400: 80}[w] for w in lengths]
    return metrics.spectral.MelSpectrogramLoss(n_mels=mels, window_lengths=lengths, mel_fmin=[0] * len(lengths),
                                               mel_fmax=[None] * len(lengths), pow=1.0, mag_weight=0.0, fused=fused)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_public_path_waveform_vs_fused_vs_unfused(kind):
    x, y = _inputs(4100)
    x64 = x.double().requires_grad_(True)
    v64 = 0.0
    for w in ([2048, 512, 64] if kind == "stft" else [32, 64, 512, 2048]):
        if kind == "stft":
            _, a, b, la, lb = _stft_formulation(x64, y, w, 2.0, torch.float64)
            v64 = v64 + (la - lb).abs().mean() + (a - b).abs().mean()
        else:
            la, lb = _mel_formulation(x64, y, w, {32: 5, 64: 10, 512: 80, 2048: 320}[w], 1.0, torch.float64)[4:]
            v64 = v64 + (la - lb).abs().mean()
    (g64,) = torch.autograd.grad(v64, x64)

    def run(fused, est_first, lengths=None):
        xa, yc = x.clone().cuda().requires_grad_(True), y.clone().cuda()
        sx, sy = A.AudioSignal(xa, SR), A.AudioSignal(yc, SR)
        loss = _public_loss(kind, fused, lengths)
        val = loss(sx, sy) if est_first else loss(sy, sx)
        (g,) = torch.autograd.grad(val, xa)
        with torch.no_grad():
            v_nograd = float(loss(sx, sy))
        return float(val), g.cpu(), (sx.stft_data, sy.stft_data), v_nograd

    for est_first in (True, False):
        (vw, gw, data, vw_ng), (v1, g1, _, v1_ng), (v0, g0, _, _) = (run(f, est_first) for f in ("waveform", True, False))
        ew, e1, e0 = (float((g - g64).abs().max() / g64.abs().max()) for g in (gw, g1, g0))
        print(f"{kind} est_first={est_first}: value waveform {vw} fused {v1} unfused {v0}; gradient err waveform {ew:.3e} "
              f"fused {e1:.3e} unfused {e0:.3e}")
        assert abs(vw - v0) <= 1e-4 * abs(v0) and vw_ng == v1_ng, "without a gradient: the code of fused=True"
        assert data == (None, None), "the waveform path leaves stft_data alone"
        assert ew <= 2 * e0 + 1e-5
    vw, v0 = (run(f, True, [2048, 400])[0] for f in ("waveform", False))      # 400: not a kernel size, runs as before
    assert abs(vw - v0) <= 1e-4 * abs(v0)


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft,T", [(512, 4100), (2048, 700001)])
@pytest.mark.parametrize("kind", KINDS)
def test_bit_equal_on_every_run(kind, n_fft, T):
    x, y = _inputs(T, "cuda")
    (s1, d1), (s2, d2) = (_kernel(kind, x, y, n_fft, 2.0, 1e-3, 1e-3, "dx") for _ in range(2))
    assert torch.equal(s1, s2) and torch.equal(d1, d2)


@pytest.mark.parametrize("kind", KINDS)
def test_waveform_on_cpu_is_the_unfused_code(kind):
    x, y = _inputs(1100)

    def run(fused):
        xa = x.clone().requires_grad_(True)
        val = _public_loss(kind, fused, [512, 64])(A.AudioSignal(xa, SR), A.AudioSignal(y.clone(), SR))
        return val.detach(), torch.autograd.grad(val, xa)[0]

    (vw, gw), (v0, g0) = run("waveform"), run(False)
    assert torch.equal(vw, v0) and torch.equal(gw, g0)


def test_argument_validation_without_gpu():
    _native.build()
    lib = _native.lib()
    p = _native.ptr(torch.zeros(4096))

    def stft(x=p, n_fft=512, hop=128, dx=p, sums=p, eps=EPS, T=4096, ws=1 << 24):
        return lib.at_stft_dist_dx_f32(x, p, 1, T, p, p, n_fft, hop, eps, 2.0, 1.0, 1.0, dx, sums, p, ws, None)

    def mel(x=p, n_fft=512, hop=128, n_mels=80, spans=p, dx=p, sums=p, eps=EPS, T=4096, ws=1 << 24):
        return lib.at_mel_dist_dx_f32(x, p, 1, T, p, p, n_fft, hop, p, p, spans, n_mels, eps, 2.0, 1.0, 1.0, dx, sums, p, ws, None)

    for call in (stft, mel):
        assert call(x=None) == -1 and call(sums=None) == -1 and call(dx=None) == -1 and call(ws=8) == -1
        assert call(n_fft=4096, hop=1024) == -2 and call(hop=100) == -2 and call(T=256) == -2 and call(eps=1e-40) == -2
    assert mel(spans=None) == -1 and mel(n_mels=129) == -2
    for nbytes, extra in ((lib.at_stft_dist_dx_workspace_bytes, ()), (lib.at_mel_dist_dx_workspace_bytes, (80,))):
        assert nbytes(0, 4096, 512, 128, *extra) == -1
        assert nbytes(1, 4096, 4096, 1024, *extra) == -2 and nbytes(1, 4096, 512, 100, *extra) == -2
        # 6 rows x 9 groups: 14 workgroups of 4 waves, each wave a partial pair and a seam slot of 3 hops; 6 x 512 margin floats
        assert nbytes(6, 4096, 512, 128, *extra) == (14 * 4 * (2 + 3 * 128) + 6 * 512) * 4
    assert lib.at_mel_dist_dx_workspace_bytes(1, 4096, 512, 128, 129) == -2
