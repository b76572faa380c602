"""GPU parity: the HIP path (through the package -> ctypes -> C-ABI) against the CPU oracle
on the same seeded inputs and against the committed golden fixtures.

Tolerances (north star): spectra / mel / filtered audio within 1e-4 relative fp32, measured PER ROW:
max|got - ref| / max|ref| over each (item, channel) row separately, the worst row counts (an
element-wise relative error is meaningless for bins near zero, and a whole-tensor maximum would let a
-30 dB item of synth.audio_batch be 30 dB worse than the claim); an all-zero reference row must be
reproduced as exact zeros.  LUFS within 0.1 LU (we assert 1e-2 LU, the reference's own FIR-vs-IIR gap).
test_*_structured_inputs add tonal / pink / swept / 100 dB-dynamic-range signals (white noise has a flat
spectrum and never exercises the dynamic range inside one frame) and bound the HIP error against float64
by the float32 error of torch's own implementation of the same operation."""
import os

import numpy as np
import pytest
import torch

import audiotools_amd as A
from audiotools_amd import _native, kernels, tables
from oracle import restate
from tests import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
REL = 1e-4


def row_errs(got, ref, lead=2):
    """max|got - ref| / max|ref| of every row (the leading `lead` dims index rows; tensors with fewer dims are one
    row).  A row whose reference is identically zero yields 0 when reproduced exactly and inf otherwise."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.ndim <= lead:
        got, ref = got.reshape(1, -1), ref.reshape(1, -1)
    else:
        got, ref = got.reshape(-1, *ref.shape[lead:]).flatten(1), ref.reshape(-1, *ref.shape[lead:]).flatten(1)
    if got.shape[1] == 0:
        return torch.zeros(got.shape[0], dtype=torch.float64)
    d = (got - ref).abs().amax(1).double()
    r = ref.abs().amax(1).double()
    return torch.where(r > 0, d / r.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))


def rel_err(got, ref, lead=2):
    e = row_errs(got, ref, lead)
    return float(e.max()) if e.numel() else 0.0


def test_native_library_is_loaded():
    """Fail loudly if the HIP library is not the thing being tested."""
    lib = _native.lib()
    assert lib is not None and os.path.exists(_native.LIB_PATH)
    with open("/proc/self/maps") as f:
        assert "libaudiotools_amd.so" in f.read()


@pytest.mark.parametrize("n_fft,hop", [(32, 8), (64, 16), (128, 32), (256, 64), (512, 128), (1024, 256), (2048, 512),
                                       (512, 100), (2048, 300)])
@pytest.mark.parametrize("wt", ["hann", "sqrt_hann"])
def test_stft_vs_oracle(n_fft, hop, wt):
    x = synth.audio_batch(3, 2, 20000, seed=n_fft + hop, gaps=False)
    s = A.AudioSignal(x.clone(), 16000).to("cuda")
    X = s.stft(n_fft, hop, wt)
    ref = restate.stft(x, n_fft, hop, wt)
    assert X.dtype == torch.complex64 and X.shape == ref.shape
    assert X.stride()[-2] == 1, "bin-contiguous physical layout (B,C,N,F) as torch.stft"
    assert rel_err(X, ref) < REL


@pytest.mark.parametrize("n_fft", [32, 64, 128, 256, 512, 1024])
@pytest.mark.parametrize("with_mel", [False, True])
def test_stft_run_stores_ragged_groups(n_fft, with_mel):
    """The wave kernels with several frames per wave (n_fft <= 1024) write a group of FW = 2048 / n_fft consecutive frames as
    one stream of 512-byte runs out of LDS (round 5).  Frame counts around the group size -- 1, FW - 1, FW, FW + 1, several
    groups + a ragged tail -- against torch.stft in float64, for three rows, with guard bands in front of and behind the
    caller-provided output buffers: a group must never write past the frames that exist."""
    from audiotools_amd import kernels, tables
    if with_mel and n_fft == 32:
        pytest.skip("the fused mel stage needs at least one 16-bin row per band group: n_fft >= 64")
    FW = 2048 // n_fft
    hop = n_fft // 4
    sr, n_mels = 16000, {32: 5, 64: 10, 128: 20, 256: 40, 512: 80, 1024: 80}[n_fft]
    dev = torch.device("cuda")
    win = tables.window("hann", n_fft, dev)
    mel = (tables.mel_units(sr, n_fft, n_mels, 0.0, None, dev) + (n_mels,)) if with_mel else None
    for n_frames in sorted({1, 2, max(FW - 1, 1), FW, FW + 1, 3 * FW + max(FW - 1, 1), 5 * FW}):
        T = max((n_frames - 1) * hop + (1 if n_frames > 1 else 0), n_fft // 2 + 1)       # 1 + T // hop frames; reflect padding needs T > n_fft / 2
        N = 1 + T // hop
        x = synth.audio_batch(3, 1, T, seed=n_fft + n_frames, gaps=False)
        F = n_fft // 2 + 1
        G = 1000
        big = torch.full((G + 3 * N * F + G,), 7.0 + 3.0j, dtype=torch.complex64, device=dev)
        sb = big[G:G + 3 * N * F].view(3, 1, N, F)
        bigm = torch.full((G + 3 * N * n_mels + G,), -5.0, device=dev)
        mb = bigm[G:G + 3 * N * n_mels].view(3, 1, N, n_mels) if with_mel else None
        X, Mm = kernels.stft_mel(x.to(dev), win, n_fft, hop, mel=mel, out=(sb, mb))
        ref = restate.stft(x.double(), n_fft, hop, "hann")
        assert X.shape == ref.shape, (n_frames, X.shape, ref.shape)
        assert rel_err(X, ref) < REL, (n_fft, n_frames)
        assert bool((big[:G] == 7.0 + 3.0j).all()) and bool((big[-G:] == 7.0 + 3.0j).all()), (n_fft, n_frames, "spectrum guard")
        if with_mel:
            refm = restate.mel_spectrogram(ref.to(torch.complex64), sr, n_mels)
            assert rel_err(Mm, refm) < REL, (n_fft, n_frames)
            assert bool((bigm[:G] == -5.0).all()) and bool((bigm[-G:] == -5.0).all()), (n_fft, n_frames, "mel guard")


@pytest.mark.parametrize("T", [16000, 16001, 15999, 4098])
def test_stft_odd_lengths_and_alignment(T):
    x = synth.audio_batch(2, 3, T, seed=T, gaps=False)
    s = A.AudioSignal(x.clone(), 16000).to("cuda")
    assert rel_err(s.stft(512, 128), restate.stft(x, 512, 128)) < REL
    assert rel_err(s.stft(512, 127, "average"), restate.stft(x, 512, 127, "average")) < REL


@pytest.mark.parametrize("padding_type", ["reflect", "constant", "replicate", "circular"])
@pytest.mark.parametrize("n_fft", [512, 2048])
def test_stft_match_stride(padding_type, n_fft):
    x = synth.audio_batch(2, 1, 30000 + 17, seed=5, gaps=False)
    s = A.AudioSignal(x.clone(), 44100).to("cuda")
    X = s.stft(n_fft, n_fft // 4, "sqrt_hann", True, padding_type)
    ref = restate.stft(x, n_fft, n_fft // 4, "sqrt_hann", True, padding_type)
    assert rel_err(X, ref) < REL
    # the reference's own property (tests/core/test_audio_signal.py:430-456): frames*hop == padded length
    hop = n_fft // 4
    assert X.shape[-1] == (x.shape[-1] + (-x.shape[-1]) % hop) // hop


def test_stft_golden_cfg1():
    d = np.load(os.path.join(G, "stft_cfg1.npz"))
    s = A.AudioSignal(torch.from_numpy(d["x"]), 16000).to("cuda")
    assert rel_err(s.stft(512, 128, "hann"), torch.from_numpy(d["stft"])) < REL
    assert rel_err(s.stft(512, 128, "sqrt_hann", match_stride=True),
                   torch.from_numpy(d["stft_match_stride_sqrt_hann"])) < REL


def test_stft_kat_f64():
    x = synth.audio_batch(8, 1, 16000, seed=1, gaps=False)
    X = A.AudioSignal(x.clone(), 16000).to("cuda").stft(512, 128, "hann").cpu().numpy()
    K = restate.stft_f64_direct(x.numpy(), 512, 128, "hann")
    assert np.abs(X - K).max() / np.abs(K).max() < 1e-5


def test_stft_linearity_and_roundtrip_full_size():
    """Size-independent properties at a BASELINE-sized row count (cfg2 per-row shape)."""
    B, C, T = 8, 2, 441000
    g = torch.Generator(device="cuda").manual_seed(3)
    a = 0.1 * torch.randn(B, C, T, device="cuda", generator=g)
    b = 0.1 * torch.randn(B, C, T, device="cuda", generator=g)
    sa, sb = A.AudioSignal(a, 44100), A.AudioSignal(b, 44100)
    Xa, Xb = sa.stft().clone(), sb.stft().clone()
    Xs = A.AudioSignal(2.0 * a - 3.0 * b, 44100).stft()
    assert Xa.shape == (B, C, 1025, 862)
    assert rel_err(Xs, 2.0 * Xa - 3.0 * Xb) < REL
    # istft(stft(x)) == x (tests/core/test_audio_signal.py:400-428)
    y = sa.istft().audio_data
    assert float((y - a).abs().max()) < 1e-5
    # Parseval per row for the hann window at 75 % overlap: sum|X|^2 ~ 1.5*n_fft*sum x^2 (interior)
    assert torch.isfinite(Xa.abs()).all()


@pytest.mark.parametrize("sr,n_fft,n_mels", [(44100, 2048, 80), (16000, 512, 80), (22050, 1024, 64), (8000, 256, 40)])
def test_mel_vs_oracle(sr, n_fft, n_mels):
    x = synth.audio_batch(3, 2, sr // 2, seed=n_mels, gaps=False)
    s = A.AudioSignal(x.clone(), sr).to("cuda")
    mel = s.mel_spectrogram(n_mels)
    X = restate.stft(x, n_fft, n_fft // 4)
    ref = restate.mel_spectrogram(X, sr, n_mels)
    assert mel.shape == ref.shape
    assert rel_err(mel, ref) < REL
    assert rel_err(s.stft_data, X) < REL      # mel_spectrogram() also refreshes stft_data
    assert rel_err(s.mfcc(n_mels=n_mels), restate.mfcc(ref)) < REL


@pytest.mark.parametrize("win,n_mels", [(32, 5), (64, 10), (128, 20), (256, 40), (512, 80), (1024, 160), (2048, 320), (2048, 5), (512, 5)])
def test_mel_loss_grid(win, n_mels):
    """The (window, n_mels) grid of metrics/spectral.py MelSpectrogramLoss.  Banks that do not fit
    the fused unit layout (very wide or very many bands) take native STFT + dense basis on the
    device -- never an error."""
    x = synth.audio_batch(2, 1, 16000, seed=win + n_mels, gaps=False)
    s = A.AudioSignal(x.clone(), 44100).to("cuda")
    got = s.mel_spectrogram(n_mels, window_length=win, hop_length=win // 4, window_type="hann")
    X_ref = restate.stft(x, win, win // 4)
    ref = restate.mel_spectrogram(X_ref, 44100, n_mels)
    assert rel_err(got, ref) < REL
    assert rel_err(torch.view_as_real(s.stft_data), torch.view_as_real(X_ref)) < REL


@pytest.mark.parametrize("op", ["low_pass", "high_pass", "equalizer"])
def test_fir_family_native_gradient_vs_float64(op):
    """low_pass / high_pass / equalizer on a HIP tensor that requires grad stay on the FIR kernels (forward kernel + the
    adjoint on the same kernel, filters._NativeFir; the reference promises gradients through them,
    tests/core/test_grad.py:44-66): value and dL/daudio against a float64 evaluation of the torch formulation."""
    from audiotools_amd import filters
    sr, T = 16000, 12000
    x = synth.audio_batch(3, 2, T, seed=77, gaps=False, sample_rate=sr)
    g = torch.Generator().manual_seed(3)
    wgt = torch.randn(3, 2, T, generator=g)
    arg = torch.tensor([1000.0, 2500.0, 4000.0]) if op != "equalizer" else -torch.rand(3, 6, generator=g)

    # float64 yardstick: the torch formulation of the same filter (the reference's float32 taps, applied in float64)
    x64 = x.double().clone().requires_grad_(True)
    if op == "equalizer":
        from audiotools_amd import fx
        taps, half = fx.equalizer_taps(sr, (10 ** arg).float())
        y64 = torch.stack([filters._conv_rows_replicate(x64[b], taps[b].double(), half) for b in range(3)])
    else:
        y64 = filters.lowpass_torch(x64, (arg / sr)[:, None], 51, op == "high_pass")
    (g64,) = torch.autograd.grad((y64 * wgt.double()).sum(), x64)
    a = x.cuda().clone().requires_grad_(True)
    y32 = getattr(A.AudioSignal(a, sr), op)(arg.clone()).audio_data
    assert "NativeFir" in type(y32.grad_fn).__name__, type(y32.grad_fn).__name__     # the kernels ran, not the torch formulation
    (g32,) = torch.autograd.grad((y32 * wgt.cuda()).sum(), a)
    assert rel_err(y32.detach(), y64.detach()) < REL
    assert rel_err(g32, g64) < REL


@pytest.mark.parametrize("old,new,T", [(44100, 16000, 30000), (16000, 44100, 9000), (48000, 44100, 20001), (16000, 8000, 777)])
def test_resample_native_gradient_vs_float64(old, new, T):
    """resample() on a HIP tensor that requires grad stays on the kernels (filters._NativeResample: forward kernel, the
    transposed polyphase sum on the VALU kernel with the rates swapped, the replicate padding folded back;
    tests/core/test_grad.py:62): value and dL/daudio against the torch formulation evaluated in float64."""
    from audiotools_amd import filters, tables
    x = synth.audio_batch(3, 2, T, seed=old % 97 + T, gaps=False, sample_rate=old)
    x64 = x.double().clone().requires_grad_(True)
    bank, o, n, width = tables.resample_bank(old, new)
    xp = torch.nn.functional.pad(x64.reshape(-1, 1, T), (width, width + o), mode="replicate")
    y64 = torch.nn.functional.conv1d(xp, bank.double()[:, None], stride=o).transpose(1, 2).reshape(3, 2, -1)[..., : n * T // o]
    wgt = torch.randn(y64.shape, generator=torch.Generator().manual_seed(5))
    (g64,) = torch.autograd.grad((y64 * wgt.double()).sum(), x64)
    a = x.cuda().clone().requires_grad_(True)
    y32 = A.AudioSignal(a, old).resample(new).audio_data
    assert "NativeResample" in type(y32.grad_fn).__name__, type(y32.grad_fn).__name__
    (g32,) = torch.autograd.grad((y32 * wgt.cuda()).sum(), a)
    assert y32.shape == y64.shape
    assert rel_err(y32.detach(), y64.detach()) < REL
    assert rel_err(g32, g64) < REL


@pytest.mark.parametrize("T,L,Cir,ir_grad", [(24000, 8000, 1, False), (24000, 8000, 1, True), (16384, 5000, 1, False),
                                             (9000, 9000, 1, False)])
def test_convolve_apply_ir_native_gradient_vs_float64(T, L, Cir, ir_grad):
    """convolve() / apply_ir() with a HIP signal that requires grad keep the native convolution (fx._NativeCircConv:
    forward kernel, adjoints = the same kernel on index-reversed operands; tests/core/test_grad.py:47-52): values and
    gradients against the rFFT formulation of effects.py:86-121 in float64."""
    sr = 16000
    x = synth.audio_batch(3, 2, T, seed=T + L, gaps=False, sample_rate=sr)
    gen = torch.Generator().manual_seed(11)
    ir = torch.randn(3, Cir, L, generator=gen) * torch.exp(-torch.arange(L) / (L / 6.0))
    ir[:, :, 37] = 3.0                                             # a clear peak away from index 0
    wgt = torch.randn(3, 2, T, generator=gen)

    def f64(xx, ii):
        ii = torch.nn.functional.pad(ii, (0, T - L))
        idx = ii.abs().argmax(-1, keepdim=True)
        ii = torch.gather(ii, -1, (torch.arange(T)[None, None] + idx) % T)
        ii = ii / ii.abs().max(-1, keepdim=True)[0].clamp(1e-5)
        return torch.fft.irfft(torch.fft.rfft(ii, T) * torch.fft.rfft(xx, T), T)

    x64, i64 = x.double().clone().requires_grad_(True), ir.double().clone().requires_grad_(True)
    y64 = f64(x64, i64)
    gx64, gi64 = torch.autograd.grad((y64 * wgt.double()).sum(), (x64, i64))
    a = x.cuda().clone().requires_grad_(True)
    b = ir.cuda().clone().requires_grad_(ir_grad)
    y32 = A.AudioSignal(a, sr).convolve(A.AudioSignal(b, sr)).audio_data
    assert "NativeCircConv" in type(y32.grad_fn).__name__, type(y32.grad_fn).__name__
    grads = torch.autograd.grad((y32 * wgt.cuda()).sum(), (a, b) if ir_grad else (a,))
    assert rel_err(y32.detach(), y64.detach()) < REL
    assert rel_err(grads[0], gx64) < REL
    if ir_grad:
        assert rel_err(grads[1], gi64) < REL
    # apply_ir = convolve + peak restoration (torch ops around the same Function)
    a2 = x.cuda().clone().requires_grad_(True)
    y_ir = A.AudioSignal(a2, sr).apply_ir(A.AudioSignal(ir.cuda().clone(), sr)).audio_data
    x64b = x.double().clone().requires_grad_(True)
    yb = f64(x64b, ir.double())
    yb = yb * (x64b.abs().amax(-1, keepdim=True).clamp(1e-8) / yb.abs().amax(-1, keepdim=True).clamp(1e-8))
    (gb,) = torch.autograd.grad((yb * wgt.double()).sum(), x64b)
    (ga,) = torch.autograd.grad((y_ir * wgt.cuda()).sum(), a2)
    assert rel_err(y_ir.detach(), yb.detach()) < REL
    assert rel_err(ga, gb) < REL


@pytest.mark.parametrize("B,C,T,wd,hd", [(3, 2, 16000, 0.1, 0.025), (2, 1, 12345, 0.064, 0.032), (1, 2, 4000, 0.03, 0.011),
                                          (4, 1, 8000, 0.5, 0.5)])
def test_collect_windows_overlap_and_add_native(B, C, T, wd, hd):
    """collect_windows / overlap_and_add on HIP tensors (at_collect_windows_f32, at_overlap_add_f32) against the
    reference's formulation -- zero_pad(hop, hop), F.unfold, permute / reshape; F.fold of the windows and of ones, division,
    trim (dsp.py:70-151) -- evaluated by torch on the CPU, including the NaN the reference leaves where no window reaches."""
    import torch.nn.functional as F
    sr = 16000
    x = synth.audio_batch(B, C, T, seed=T, gaps=False, sample_rate=sr)
    win, hop = int(wd * sr), int(hd * sr)
    if win % hop:
        win = (win // hop) * hop
    xp = F.pad(x, (hop, hop))
    Tp = xp.shape[-1]
    unf = F.unfold(xp.reshape(-1, 1, 1, Tp), kernel_size=(1, win), stride=(1, hop))
    ref_w = unf.permute(0, 2, 1).reshape(-1, 1, win)
    s = A.AudioSignal(x.clone(), sr).to("cuda")
    s.collect_windows(wd, hd)
    assert s.audio_data.shape == ref_w.shape and torch.equal(s.audio_data.cpu(), ref_w)
    # a per-window gain so that the overlap-add is not the identity
    gain = 1.0 + 0.1 * torch.arange(ref_w.shape[0], dtype=torch.float32)[:, None, None] / ref_w.shape[0]
    s.audio_data = s.audio_data * gain.cuda()
    u = (ref_w * gain).reshape(B * C, -1, win).permute(0, 2, 1)
    kw = dict(output_size=(1, Tp), kernel_size=(1, win), stride=(1, hop))
    ref = (F.fold(u, **kw) / F.fold(torch.ones_like(u), **kw)).reshape(B, C, -1)[..., hop:-hop]
    y = s.overlap_and_add(hd).audio_data.cpu()
    assert y.shape == ref.shape
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(y), nan)
    assert float((y[~nan] - ref[~nan]).abs().max()) <= 1e-6 * float(ref[~nan].abs().max())


def test_mel_generic_size_short_clip_falls_back_to_dense_basis():
    """mel_spectrogram on generic transform sizes (4096 @ 96 kHz ...) goes to the banded mel stage of the TILED
    kernel; a clip that kernel does not take (shorter than its two-frame tile: T < n_fft + hop) must keep working through
    native stft() + the dense basis, not raise."""
    sr, n_fft, hop = 96000, 4096, 1024
    for T in (3000, 4096 + 512, 4096 + 1024 + 8, 20000):
        x = synth.audio_batch(2, 1, T, seed=T, gaps=False, sample_rate=sr)
        s = A.AudioSignal(x.clone(), sr).to("cuda")
        mel = s.mel_spectrogram(80)
        X = restate.stft(x, n_fft, hop)
        assert rel_err(mel, restate.mel_spectrogram(X, sr, 80)) < REL, T
        assert rel_err(s.stft_data, X) < REL, T


def test_mel_golden_cfg2():
    d = np.load(os.path.join(G, "mel_cfg2.npz"))
    s = A.AudioSignal(torch.from_numpy(d["x"]), 44100).to("cuda")
    assert rel_err(s.mel_spectrogram(80), torch.from_numpy(d["mel"])) < REL
    assert rel_err(s.stft_data, torch.from_numpy(d["stft"])) < REL
    assert rel_err(A.AudioSignal(torch.from_numpy(d["x"]), 44100).to("cuda").mfcc(), torch.from_numpy(d["mfcc"])) < REL


def test_mel_options():
    x = synth.audio_batch(2, 1, 22050, seed=9, gaps=False)
    s = A.AudioSignal(x.clone(), 44100).to("cuda")
    mel = s.mel_spectrogram(64, mel_fmin=50.0, mel_fmax=8000.0, window_length=1024, hop_length=256)
    ref = restate.mel_spectrogram(restate.stft(x, 1024, 256), 44100, 64, 50.0, 8000.0)
    assert rel_err(mel, ref) < REL
    # the n_fft 2048 / hop 512 kernel with banks of other sizes: a band-limited bank is 128 units (TWO rounds of its
    # cross-frame round pipeline instead of the four of the 80-band default); runs of several frames, a row end inside a run
    from audiotools_amd import tables
    X = restate.stft(x, 2048, 512)
    for n_mels, fmin, fmax in [(40, 0.0, 4000.0), (64, 200.0, 6000.0), (128, 0.0, None), (32, 0.0, None)]:
        units = tables.mel_units(44100, 2048, n_mels, fmin, fmax, torch.device("cpu"))
        assert units is not None and units[0].shape[0] in (128, 256, 384), (n_mels, fmin, fmax)
        mel = s.mel_spectrogram(n_mels, mel_fmin=fmin, mel_fmax=fmax)
        ref = restate.mel_spectrogram(X, 44100, n_mels, fmin, fmax)
        assert mel.shape == ref.shape and rel_err(mel, ref) < REL, (n_mels, fmin, fmax, units[0].shape[0])
    assert tables.mel_units(44100, 2048, 40, 0.0, 4000.0, torch.device("cpu"))[0].shape[0] == 128


# ------------------------------------------------------------------------- loudness
LU = 1e-2


def test_loudness_golden():
    d = np.load(os.path.join(G, "loudness.npz"))
    np.random.seed(0)
    arr = torch.from_numpy(np.random.randn(16, 2, 16000).astype(np.float32))
    got = A.AudioSignal(arr, 16000).to("cuda").loudness().cpu().numpy()
    assert np.abs(got - d["seeded_randn_16k"]).max() < LU
    xg = torch.from_numpy(d["gaps_x"].astype(np.float32))
    got = A.AudioSignal(xg, 16000).to("cuda").loudness().cpu().numpy()
    assert np.abs(got - d["gaps_lufs"]).max() < LU
    assert got[1] == -70.0
    for fc, key in (("Fenton/Lee 1", "fenton_lee_1"), ("Dash et al.", "dash")):
        got = A.AudioSignal(xg[:2, :, :32000].clone(), 16000).to("cuda").loudness(filter_class=fc).cpu().numpy()
        assert np.abs(got - d[key]).max() < LU
    # the reference's literal sine_1000.wav target (tests/core/test_loudness.py:61, ATOL 0.1)
    sine = synth.sine(1000, 44100, 20.0, amp=0.99924)
    got = float(A.AudioSignal(sine, 44100).to("cuda").loudness()[0])
    assert abs(got - (-3.0523438444331137)) < 1e-2


@pytest.mark.parametrize("sr,dur,C", [(44100, 10.0, 2), (48000, 3.0, 1), (16000, 0.3, 2), (22050, 1.7, 3),
                                      (11025, 2.0, 2), (44100, 0.41, 5)])
def test_loudness_vs_oracle(sr, dur, C):
    """Includes rates where K != 4*S (11025: general block path), short (<0.5 s: zero-padded)
    and barely-one-block signals, odd lengths (scalar load path)."""
    T = int(sr * dur) + (1 if sr == 22050 else 0)
    x = synth.audio_batch(5, C, T, seed=sr % 1000, sample_rate=sr)
    got = A.AudioSignal(x.clone(), sr).to("cuda").loudness().cpu()
    ref = restate.loudness(x, sr)
    assert float((got - ref).abs().max()) < LU, (got, ref)


def test_loudness_ebu_tech_3341_cases_gpu():
    """The LUFS kernel against PUBLISHED readings (EBU Tech 3341 minimum-requirement signals 1, 2, 3,
    5; tolerance +-0.1 LU), all four signals in one batch (zero padding to the longest is part of
    the check: trailing silence is gated out)."""
    from tests.test_leaf_pins import _tone
    sr = 48000
    sigs = [_tone(-23.0, 20), _tone(-33.0, 20),
            torch.cat([_tone(-36.0, 10), _tone(-23.0, 60), _tone(-36.0, 10)]),
            torch.cat([_tone(-26.0, 20), _tone(-20.0, 20.1), _tone(-26.0, 20)])]
    want = [-23.0, -33.0, -23.0, -23.0]
    for s_, w in zip(sigs, want):
        x = s_[None, None].repeat(1, 2, 1)
        got = float(A.AudioSignal(x, sr).to("cuda").loudness()[0])
        assert abs(got - w) < 0.1, (got, w)
    T = max(s_.numel() for s_ in sigs)
    xb = torch.stack([torch.nn.functional.pad(s_, (0, T - s_.numel())) for s_ in sigs])[:, None].repeat(1, 2, 1)
    got = A.AudioSignal(xb, sr).to("cuda").loudness().cpu()
    assert float((got - torch.tensor(want)).abs().max()) < 0.1, got


def test_loudness_meter_api_and_cache():
    x = synth.audio_batch(4, 2, 2 * 44100, seed=2, gaps=False)
    m = A.Meter(44100).to("cuda")
    got = m.integrated_loudness(x.cuda().permute(0, 2, 1))
    ref = restate.integrated_loudness(x, 44100)
    assert float((got.cpu() - ref).abs().max()) < LU
    s = A.AudioSignal(x.clone(), 44100).to("cuda")
    l1 = s.loudness()
    assert s.loudness() is not None and torch.equal(s.loudness(), l1)
    s.audio_data = s.audio_data * 0.5
    assert abs(float((s.loudness() - l1)[0]) + 6.0206) < 1e-2     # -6.02 dB, linearity of the meter


def test_loudness_segmentation_invariance():
    """Rows are split into independently filtered segments with a warm-up; the result must not
    depend on the batch size that drives the segmentation heuristic."""
    x = synth.audio_batch(1, 2, 30 * 44100, seed=77, sample_rate=44100)
    one = A.AudioSignal(x.clone(), 44100).to("cuda").loudness().cpu()
    many = A.AudioSignal(x.repeat(64, 1, 1), 44100).to("cuda").loudness().cpu()
    ref = restate.loudness(x, 44100)
    assert float((one - ref).abs().max()) < LU
    assert float((many - one).abs().max()) < 1e-4


# ------------------------------------------------------- FIR / resample / convolve rows
def test_effects_golden_cfg4():
    d = np.load(os.path.join(G, "effects_cfg4.npz"))
    x = torch.from_numpy(d["x"])
    s = lambda: A.AudioSignal(x.clone(), 48000).to("cuda")
    assert rel_err(s().low_pass(torch.from_numpy(d["lp_cut"])).audio_data, torch.from_numpy(d["low_pass"])) < REL
    assert rel_err(s().high_pass(torch.tensor([500.0, 1000.0, 2000.0])).audio_data, torch.from_numpy(d["high_pass"])) < REL
    assert rel_err(s().equalizer(torch.from_numpy(d["eq_db"])).audio_data, torch.from_numpy(d["equalizer"])) < REL
    ir = A.AudioSignal(torch.from_numpy(d["ir"]).clone(), 48000).to("cuda")
    assert rel_err(s().convolve(ir).audio_data, torch.from_numpy(d["convolve"])) < REL
    assert rel_err(s().resample(16000).audio_data, torch.from_numpy(d["resample_48k_16k"])) < REL
    xr = torch.from_numpy(d["xr"])
    assert rel_err(A.AudioSignal(xr, 44100).to("cuda").resample(16000).audio_data, torch.from_numpy(d["resample_441_16k"])) < REL


@pytest.mark.parametrize("highpass", [False, True])
def test_sinc_filters_vs_oracle(highpass):
    """Per-item cutoffs incl. a very long filter (50 Hz -> 44 983 taps) and odd lengths."""
    x = synth.audio_batch(4, 2, 30001, seed=31, gaps=False)
    cut = torch.tensor([4000.0, 16000.0, 300.0, 50.0])
    s = A.AudioSignal(x.clone(), 44100).to("cuda")
    got = (s.high_pass(cut) if highpass else s.low_pass(cut)).audio_data
    ref = restate.high_pass(x, cut, 44100) if highpass else restate.low_pass(x, cut, 44100)
    assert rel_err(got, ref) < REL
    assert s.stft_data is None


@pytest.mark.parametrize("L", [9, 97, 613, 1047, 1535, 1537, 3001])
@pytest.mark.parametrize("highpass", [False, True])
def test_fir_direct_and_fft_forms(L, highpass):
    """Both native FIR forms (register-window direct, overlap-save block FFT incl. the partitioned
    case L > 1536) against float64 conv1d with replicate padding; asymmetric per-item taps, odd T."""
    from audiotools_amd import kernels
    B, C, T = 3, 2, 10007
    g = torch.Generator().manual_seed(L)
    x = torch.randn(B, C, T, generator=g)
    taps = torch.randn(B, L, generator=g) / L ** 0.5
    half = (L - 1) // 2
    xp = torch.nn.functional.pad(x.double(), (half, half), mode="replicate")
    ref = torch.stack([torch.nn.functional.conv1d(xp[b][:, None], taps[b].double()[None, None])[:, 0] for b in range(B)])
    if highpass:
        ref = x.double() - ref
    for method in ("direct", "fft"):
        got = kernels.fir_per_item(x.cuda(), taps.cuda(), highpass=highpass, method=method)
        assert rel_err(got, ref.float()) < REL, method
    shared = kernels.fir_per_item(x.cuda(), taps[:1].cuda(), highpass=highpass, method="fft")
    ref0 = torch.nn.functional.conv1d(xp.reshape(-1, 1, xp.shape[-1]), taps[0].double()[None, None]).reshape(B, C, T)
    assert rel_err(shared, ((x.double() - ref0) if highpass else ref0).float()) < REL


@pytest.mark.parametrize("L,T", [(6145, 10007), (9001, 30000), (44983, 30001)])
@pytest.mark.parametrize("highpass", [False, True])
def test_fir_long_form(L, T, highpass):
    """Filters of thousands of taps (HighPass's default 50 / 100 / 250 Hz cutoffs at 44.1 kHz: 44 983 / 22 491 / 8 997 taps)
    run as ONE circular convolution by the four-step FFT instead of one overlap-save pass per 1024 taps
    (kernels._fir_long): against float64 conv1d with replicate padding, asymmetric per-item and shared taps, taps longer
    than the signal, and against the overlap-save form."""
    from audiotools_amd import kernels
    B, C = 3, 2
    g = torch.Generator().manual_seed(L + T)
    x = torch.randn(B, C, T, generator=g)
    taps = torch.randn(B, L, generator=g) / L ** 0.5
    half = (L - 1) // 2
    xp = torch.nn.functional.pad(x.double(), (half, half), mode="replicate")

    def corr64(h):        # float64 conv1d(xp, h) (a correlation) through FFTs: 1e-13 of the direct sum, which takes minutes at 45 k taps
        n = 1 << (xp.shape[-1] + L).bit_length()
        return torch.fft.irfft(torch.fft.rfft(xp, n) * torch.fft.rfft(h.double().flip(-1), n), n)[..., L - 1: L - 1 + T]

    ref = corr64(taps[:, None, :])
    if highpass:
        ref = x.double() - ref
    auto = kernels.fir_per_item(x.cuda(), taps.cuda(), highpass=highpass)            # "auto" picks the long form here
    long_ = kernels.fir_per_item(x.cuda(), taps.cuda(), highpass=highpass, method="long")
    fft = kernels.fir_per_item(x.cuda(), taps.cuda(), highpass=highpass, method="fft")
    assert torch.equal(auto, long_)
    assert rel_err(long_, ref.float()) < REL and rel_err(fft, ref.float()) < REL
    shared = kernels.fir_per_item(x.cuda(), taps[:1].cuda(), highpass=highpass, method="long")
    ref0 = corr64(taps[0])
    assert rel_err(shared, ((x.double() - ref0) if highpass else ref0).float()) < REL
    buf = torch.empty_like(auto)
    assert kernels.fir_per_item(x.cuda(), taps.cuda(), highpass=highpass, out=buf) is buf and torch.equal(buf, auto)


@pytest.mark.parametrize("mulaw", [False, True])
def test_quantization_kernel_equals_the_torch_chain(mulaw):
    """quantization / mulaw_quantization on HIP tensors run as one kernel (at_quantize_f32) that performs the reference's
    chain one float32 operation at a time (effects.py:452-527).  Against the same chain run by torch on the device and on
    the CPU: equal except where a transcendental's last bit moves a sample across a level boundary (< 1e-4 of the samples,
    one level apart)."""
    g = torch.Generator().manual_seed(17)
    x = (0.5 * torch.randn(5, 2, 40000, generator=g)).clamp_(-1, 1)
    x[0, 0, :6] = torch.tensor([1.0, -1.0, 0.0, -0.0, 1e-8, -1e-8])
    ch = torch.tensor([8, 256, 32, 3, 65536])

    def chain(a, q):
        if not mulaw:
            v = ((a + 1) / 2 * q).floor() / q
            v = 2 * v - 1
        else:
            mu = q - 1.0
            v = torch.sign(a) * torch.log1p(mu * torch.abs(a)) / torch.log1p(mu)
            v = ((v + 1) / 2 * mu + 0.5).to(torch.int64)
            v = (v / mu) * 2 - 1.0
            v = torch.sign(v) * (torch.exp(torch.abs(v) * torch.log1p(mu)) - 1.0) / mu
        return a - (a - v)

    s = A.AudioSignal(x.clone(), 16000).to("cuda")
    got = (s.mulaw_quantization(ch.clone()) if mulaw else s.quantization(ch.clone())).audio_data.cpu()
    for ref in (chain(x.cuda(), ch.cuda()[:, None, None]).cpu(), chain(x, ch[:, None, None])):
        step = 2.0 / (ch[:, None, None].float() - (1.0 if mulaw else 0.0))
        diff = (got - ref).abs()
        off = diff > 1e-6
        assert float(off.float().mean()) < 1e-4
        if not mulaw:
            assert bool((diff <= step * 1.001 + 1e-6).all())
    one = A.AudioSignal(x.clone(), 16000).to("cuda")
    same = (one.mulaw_quantization(8) if mulaw else one.quantization(8)).audio_data.cpu()     # one setting for the batch
    assert float(((same - chain(x, torch.tensor(8.0))).abs() > 1e-6).float().mean()) < 1e-4


def test_reference_dsp_properties_gpu():
    """tests/core/test_dsp.py:76-109 on the HIP path."""
    sr, f = 44100, 440
    t = torch.arange(0, 1, 1 / sr)
    sw = (torch.sin(2 * np.pi * f * t) * restate.get_window("hann", t.shape[-1]))[None, None]
    sig = A.AudioSignal(sw.repeat(3, 1, 1), sr).to("cuda")
    out = sig.clone().low_pass(torch.tensor([220.0, 880.0, 220.0])).audio_data
    assert out[0].abs().max() < 1e-4 and out[2].abs().max() < 1e-4
    assert (out[1] - sig.audio_data[1]).abs().max() < 1e-3
    assert (sig.clone().high_pass(220).audio_data - sig.audio_data).abs().max() < 1e-4
    with pytest.raises(ValueError):
        sig.clone().low_pass(30000.0)


@pytest.mark.parametrize("old,new", [(44100, 16000), (16000, 44100), (48000, 44100), (44100, 22050), (16000, 8000), (44100, 48000)])
def test_resample_vs_oracle(old, new):
    x = synth.audio_batch(3, 2, old // 2 + 13, seed=old % 97, gaps=False)
    got = A.AudioSignal(x.clone(), old).to("cuda").resample(new)
    ref = restate.resample(x, old, new)
    assert got.sample_rate == new and got.audio_data.shape == ref.shape
    assert rel_err(got.audio_data, ref) < REL


def test_equalizer_and_filterbank_properties():
    """tests/core/test_effects.py:184-231: zero-dB EQ is the identity; per-item curves match the oracle."""
    x = synth.audio_batch(3, 2, 24000, seed=41, gaps=False)
    s = A.AudioSignal(x.clone(), 44100).to("cuda")
    assert float((s.clone().equalizer(torch.zeros(3, 6)).audio_data.cpu() - x).abs().max()) < 1e-5
    db = -torch.rand(3, 8, generator=torch.Generator().manual_seed(2))
    assert rel_err(s.clone().equalizer(db).audio_data, restate.equalizer(x, 44100, db)) < REL
    fb = s.clone().mel_filterbank(8)
    assert float((fb.sum(-1).cpu() - x).abs().max()) < 1e-5
    # the native band split (one FIR per band with difference taps, effects.py:399-403) against the oracle's
    # julius.SplitBands restatement, band by band, 1 / 2 / 6 / 8 bands at two rates
    for sr, nb in ((44100, 8), (48000, 6), (16000, 2), (16000, 1)):
        got = A.AudioSignal(x.clone(), sr).to("cuda").mel_filterbank(nb)
        ref = restate.mel_filterbank(x, sr, nb)
        assert got.shape == ref.shape == (3, 2, 24000, nb)
        assert rel_err(got.permute(0, 1, 3, 2), ref.permute(0, 1, 3, 2), lead=3) < REL, (sr, nb)   # every band its own row


@pytest.mark.parametrize("T", [16, 126, 4096, 8192, 12288, 9600, 44100, 24000, 2 * 81 * 1225, 240000])
def test_fourstep_convolution_vs_float64(T):
    """csrc/longconv.hip (column FFTs, row-pair kernel, column FFTs back) against a float64 FFT
    convolution and against the rocFFT engine: N1 = 1 (one row, self-paired), even and odd N1
    (self-paired middle row or not), radix 7, partial column tiles, per-item scale, Cir = 1 / C."""
    from audiotools_amd import kernels
    assert kernels.longconv_supported(T)
    B, C = (2, 2) if T > 50000 else (3, 2)
    g = torch.Generator().manual_seed(T % 97)
    x = torch.randn(B, C, T, generator=g)
    for Cir in (1, C):
        ir = torch.randn(B, Cir, T, generator=g) * torch.exp(-torch.arange(T) / (0.2 * T))
        scale = torch.rand(B, Cir, 1, generator=g) + 0.5
        ref = torch.fft.irfft(torch.fft.rfft(x.double()) * torch.fft.rfft(ir.double()), n=T) * scale.double()
        got = kernels.fftconv(x.cuda(), ir.cuda(), scale.cuda(), engine="fourstep")
        roc = kernels.fftconv(x.cuda(), ir.cuda(), scale.cuda(), engine="rocfft")
        e4, er = rel_err(got.double(), ref), rel_err(roc.double(), ref)
        assert e4 < 2e-6, (T, Cir, e4, er)
        assert e4 < 4 * er + 2e-7, (T, Cir, e4, er)       # as accurate as the library transform
    # unit impulse at an odd delay: a circular shift, exactly representable
    imp = torch.zeros(B, 1, T)
    imp[..., 7 % T] = 1
    back = kernels.fftconv(x.cuda(), imp.cuda(), None, engine="fourstep")
    assert float((back.cpu() - torch.roll(x, 7 % T, -1)).abs().max()) < 2e-5


@pytest.mark.parametrize("T,L", [(24000, 9601), (9600, 9600), (12288, 20000), (44100, 1)])
def test_room_convolution_fused_roll_and_peaks(T, L):
    """at_longconv_room_f32: zero padding + roll to the peak inside the load of the IR transform (odd
    shifts, IR shorter / equal / longer than the signal, one-sample IR), and the two peaks of
    apply_ir found inside the transforms -- against the unfused path (absmax, roll_pad, rocFFT)."""
    g = torch.Generator().manual_seed(L % 31)
    B, C = 3, 2
    x = torch.randn(B, C, T, generator=g)
    ir = torch.randn(B, 1, L, generator=g) * torch.exp(-torch.arange(L) / (0.3 * L + 1))
    for b in range(B):                                  # distinct, odd and even peak positions
        ir[b, 0, (37 * b + 5) % L] = 9.0 + b
    Lc = min(L, T)
    raw = ir[..., :Lc].contiguous().cuda()
    peak, idx = kernels.absmax(raw, want_index=True)
    scale = 1 / peak[..., None].clamp(1e-5)
    got, xpk, ypk = kernels.room_convolve(x.cuda(), raw, idx, scale, want_peaks=True)
    rolled = kernels.roll_pad(raw, idx, T)
    ref = kernels.fftconv(x.cuda(), rolled, scale, engine="rocfft")
    ref64 = torch.fft.irfft(torch.fft.rfft(x.double()) * torch.fft.rfft(rolled.cpu().double()), n=T) * scale.cpu().double()
    assert rel_err(got.double(), ref64) < 2e-6 and rel_err(got, ref) < 5e-6
    assert torch.equal(xpk.cpu(), x.abs().amax(-1))
    assert torch.equal(ypk, got.abs().amax(-1))
    # no shift, no peaks, multi-channel IR
    ir2 = torch.randn(B, C, Lc, generator=g)
    got2 = kernels.room_convolve(x.cuda(), ir2.cuda(), None, None)
    ref2 = torch.fft.irfft(torch.fft.rfft(x.double()) * torch.fft.rfft(torch.nn.functional.pad(ir2, (0, T - Lc)).double()), n=T)
    assert rel_err(got2.double(), ref2) < 2e-6
    # the AudioSignal methods: convolve / apply_ir through the fused path == the CPU formulation
    mk = lambda dev: (A.AudioSignal(x.clone(), 16000).to(dev), A.AudioSignal(ir.clone(), 16000).to(dev))
    sg, ig = mk("cuda")
    sc, ic = mk("cpu")
    assert rel_err(sg.clone().convolve(ig.clone()).audio_data, sc.clone().convolve(ic.clone()).audio_data) < REL
    yg = sg.clone().apply_ir(ig, drr=torch.tensor([3.0, 8.0, 12.0]))
    yc = sc.clone().apply_ir(ic, drr=torch.tensor([3.0, 8.0, 12.0]))
    assert rel_err(yg.audio_data, yc.audio_data) < 2e-4
    assert ig.signal_length == ic.signal_length                       # the in-place pad / truncate of the argument
    # NaN in the input reaches both peaks (as at_absmax_f32 propagates it)
    xn = x.clone()
    xn[1, 0, 5] = float("nan")
    _, xpk, ypk = kernels.room_convolve(xn.cuda(), raw, idx, scale, want_peaks=True)
    assert torch.isnan(xpk[1, 0]) and torch.isnan(ypk[1, 0]) and not torch.isnan(xpk[0]).any()


def test_fourstep_is_the_default_engine(monkeypatch):
    from audiotools_amd import kernels
    x = torch.randn(2, 1, 48000, device="cuda")
    ir = torch.randn(2, 1, 48000, device="cuda")
    called = []
    lib = _native.lib()
    orig = lib.at_longconv_circ_f32
    class Spy:
        def __call__(self, *a):
            called.append(1)
            return orig(*a)
    monkeypatch.setattr(lib, "at_longconv_circ_f32", Spy(), raising=False)
    kernels.fftconv(x, ir)
    assert called
    assert not kernels.longconv_supported(10007) and not kernels.longconv_supported(2 * 11 * 64)
    kernels.fftconv(torch.randn(1, 1, 10007, device="cuda"), torch.randn(1, 1, 10007, device="cuda"))   # rocFFT path still there


@pytest.mark.parametrize("T,Lir", [(24000, 9600), (16000, 16000), (10007, 20000)])
def test_convolve_vs_oracle(T, Lir):
    """Circular FFT convolution incl. a prime length (Bluestein in rocFFT) and IR longer than the signal."""
    x = synth.audio_batch(3, 2, T, seed=T % 89, gaps=False)
    g = torch.Generator().manual_seed(7)
    ir = torch.randn(3, 1, Lir, generator=g) * torch.exp(-torch.arange(Lir) / (0.1 * Lir))
    got = A.AudioSignal(x.clone(), 16000).to("cuda").convolve(A.AudioSignal(ir.clone(), 16000).to("cuda"))
    assert rel_err(got.audio_data, restate.convolve(x, ir)) < REL
    # identity: (delayed) unit impulse returns the input (tests/core/test_effects.py:86-121)
    imp = torch.zeros(3, 1, T)
    imp[..., 777] = 1
    back = A.AudioSignal(x.clone(), 16000).to("cuda").convolve(A.AudioSignal(imp, 16000).to("cuda"))
    assert float((back.audio_data.cpu() - x).abs().max()) < 1e-5


def test_apply_ir_and_normalize():
    x = synth.audio_batch(3, 1, 32000, seed=51, gaps=False, sample_rate=16000)
    g = torch.Generator().manual_seed(8)
    ir = torch.randn(3, 1, 8000, generator=g) * torch.exp(-torch.arange(8000) / 1500.0)
    s = A.AudioSignal(x.clone(), 16000).to("cuda")
    y = s.clone().apply_ir(A.AudioSignal(ir.clone(), 16000).to("cuda"), drr=torch.tensor([5.0, 10.0, 15.0]),
                           ir_eq=-torch.rand(3, 6, generator=g))
    # apply_ir restores the input peak (effects.py:175-177)
    assert torch.allclose(y.audio_data.abs().amax(-1), s.audio_data.abs().amax(-1), rtol=1e-4)
    n = s.clone().normalize(-30.0)
    assert float((n.loudness().cpu() + 30.0).abs().max()) < 0.1


def test_ir_tools_vs_torch_path():
    """at_absmax_f32 / at_roll_pad_f32 / at_alter_drr_f32 against the torch formulation of the same
    methods on CPU (which tests/test_transforms.py pins to the unmodified reference)."""
    from audiotools_amd import kernels, fx
    g = torch.Generator().manual_seed(77)
    for C, T in ((1, 9601), (2, 4099)):
        ir = torch.randn(4, C, T, generator=g) * torch.exp(-torch.arange(T) / (0.2 * T))
        ir[1, 0, 500] = ir[1].abs().max() * 1.5       # a clear direct path
        ir[2, 0, 100] = 3.0
        ir[2, 0, 200] = -3.0                            # |peak| tie: the first index wins
        v, i = kernels.absmax(ir.cuda(), want_index=True)
        assert torch.equal(v.cpu(), ir.abs().max(-1).values)
        assert torch.equal(i.cpu(), ir.abs().argmax(-1))
        if C == 1:
            rolled = kernels.roll_pad(ir.cuda(), i, T + 777)
            ref = fx._roll_to_peak(torch.nn.functional.pad(ir, (0, 777)))
            assert torch.equal(rolled.cpu(), ref)
            assert torch.equal(kernels.roll_pad(ir.cuda(), None, T - 100).cpu(), ir[..., : T - 100])
        drr = torch.tensor([0.0, 10.0, 20.0, 30.0])
        ref = A.AudioSignal(ir.clone(), 48000).alter_drr(drr).audio_data
        got = A.AudioSignal(ir.clone(), 48000).to("cuda").alter_drr(drr).audio_data.cpu()
        # (channels whose early span misses the channel-0 window can have no real root: NaN rows,
        #  in the reference too)
        assert torch.equal(torch.isnan(got), torch.isnan(ref))
        assert rel_err(torch.nan_to_num(got), torch.nan_to_num(ref)) < 1e-5
    # whole apply_ir chain (ir EQ, DRR change, rotation, FFT convolution, peak restore) vs the CPU path
    x = synth.audio_batch(3, 1, 24000, seed=5, gaps=False, sample_rate=16000)
    ir = torch.randn(3, 1, 8000, generator=g) * torch.exp(-torch.arange(8000) / 1500.0)
    eq = -torch.rand(3, 6, generator=g)
    mk = lambda dev: A.AudioSignal(x.clone(), 16000).to(dev).apply_ir(
        A.AudioSignal(ir.clone(), 16000).to(dev), drr=torch.tensor([5.0, 10.0, 15.0]), ir_eq=eq.clone()).audio_data
    assert rel_err(mk("cuda"), mk("cpu")) < REL


def test_spectral_edits_vs_torch_path():
    """at_spec_mask_f32 / at_spec_phase_shift_f32 / at_spec_mask_lowmag_f32 (dsp.py:217-352) against
    the reference's polar formulation run on CPU by the same methods (pinned to the unmodified
    reference by tests/test_transforms.py), scalar and per-item parameters."""
    x = synth.audio_batch(3, 2, 16000 + 3, seed=61, gaps=False, sample_rate=16000)

    def pair():
        a = A.AudioSignal(x.clone(), 16000, stft_params=A.STFTParams(512, 128)).to("cuda")
        b = A.AudioSignal(x.clone(), 16000, stft_params=A.STFTParams(512, 128))
        a.stft(); b.stft()
        return a, b

    cases = [
        ("mask_frequencies", dict(fmin_hz=1000.0, fmax_hz=2500.0)),
        ("mask_frequencies", dict(fmin_hz=torch.tensor([0.0, 500.0, 4000.0]), fmax_hz=torch.tensor([100.0, 7000.0, 8000.0]), val=0.5)),
        ("mask_timesteps", dict(tmin_s=0.2, tmax_s=0.5)),
        ("mask_timesteps", dict(tmin_s=torch.tensor([0.0, 0.3, 0.9]), tmax_s=torch.tensor([0.1, 0.6, 1.1]), val=0.25)),
        ("shift_phase", dict(shift=np.pi)),
        ("shift_phase", dict(shift=torch.tensor([0.3, -1.2, 2.0]))),
    ]
    for name, kw in cases:
        a, b = pair()
        before = a.stft_data
        keep = before.clone()
        getattr(a, name)(**kw); getattr(b, name)(**kw)
        assert a.stft_data is not before and torch.equal(before, keep)      # a NEW tensor, like the reference
        assert rel_err(torch.view_as_real(a.stft_data), torch.view_as_real(b.stft_data)) < 1e-5, name
        assert rel_err(a.istft().audio_data, b.istft().audio_data) < REL, name
    # mask_low_magnitudes: the mask is a threshold on a float32 log; allow a vanishing number of
    # threshold flips from 1-ulp differences in |X| between devices
    for cut in (-10.0, torch.tensor([-20.0, 0.0, 10.0])):
        a, b = pair()
        a.mask_low_magnitudes(cut); b.mask_low_magnitudes(cut)
        ga, gb = a.stft_data.cpu(), b.stft_data
        flips = ((ga.abs() == 0) != (gb.abs() == 0)).float().mean()
        assert float(flips) < 1e-4
        same = (ga.abs() == 0) == (gb.abs() == 0)
        assert float((ga - gb)[same].abs().max() / gb.abs().max()) < 1e-5
        assert 0.01 < float((ga.abs() == 0).float().mean()) < 0.99


@pytest.mark.parametrize("win,hop,T", [(2048, 512, 22050 + 7), (512, 128, 16000), (1024, 512, 12001), (256, 16, 5000), (64, 8, 1000)])
def test_stft_autograd_native_adjoint(win, hop, T):
    """Gradients through the native stft() (forward kernel + at_stft_adjoint_f32) equal those of
    torch.stft on CPU -- the path of metrics/spectral.py's losses (MultiScaleSTFTLoss,
    MelSpectrogramLoss) and tests/core/test_grad.py."""
    x = synth.audio_batch(2, 2, T, seed=win + T, gaps=False)
    g = torch.Generator().manual_seed(3)

    def loss_and_grad(dev):
        xa = x.clone().to(dev).requires_grad_(True)
        s = A.AudioSignal(xa, 44100)
        X = s.stft(win, hop, "hann")
        wts = torch.randn(X.shape, generator=torch.Generator().manual_seed(5)).to(dev)
        # magnitude, log-magnitude and raw complex terms, as the spectral losses use them
        loss = (X.abs() * wts).sum() + (X.abs().clamp(1e-5).log10() * wts).mean() + (X.real * wts + X.imag * wts.flip(-1)).sum()
        mel = s.mel_spectrogram(20, window_length=win, hop_length=hop, window_type="hann")
        loss = loss + mel.clamp(1e-5).log10().mean()
        (gx,) = torch.autograd.grad(loss, xa)
        return float(loss), gx

    l_ref, g_ref = loss_and_grad("cpu")
    l_got, g_got = loss_and_grad("cuda")
    assert abs(l_got - l_ref) <= 1e-4 * abs(l_ref)
    assert rel_err(g_got, g_ref) < REL
    with open("/proc/self/maps") as f:
        assert "libaudiotools_amd.so" in f.read()


@pytest.mark.parametrize("win,hop,T,ms,ptype", [(4096, 1024, 30000, False, None), (8192, 2048, 50000, False, None), (400, 100, 9000, False, None),
                                                 (1200, 300, 16001, False, None), (1920, 480, 20000, False, None),
                                                 (2048, 512, 22050 + 7, True, None), (512, 128, 16000, True, "constant"),
                                                 (400, 100, 9001, True, None), (4096, 1024, 30000, True, "replicate"),
                                                 (1024, 256, 12000, True, "circular"), (400, 160, 9000, False, None)])
def test_stft_autograd_general_adjoint(win, hop, T, ms, ptype):
    """the run-time transform sizes (4096 / 8192, the speech windows) and match_stride keep the HIP
    kernels under autograd -- forward = the no-grad kernel, backward = kernels.stft_adjoint_general (inverse kernels with the
    envelope division undone / at_stft_adjoint_f32, edge frames as zero frames, both paddings folded back).  grad_fn is
    asserted native; the gradient is held against float64 torch on the CPU at 1e-4 per row (metrics/spectral.py:9-247,
    tests/core/test_grad.py:44-66)."""
    x = synth.audio_batch(2, 2, T, seed=win + T, gaps=False)
    kw = dict(window_length=win, hop_length=hop, window_type="hann", match_stride=ms)
    if ptype:
        kw["padding_type"] = ptype

    def loss_and_grad(dev, dtype):
        xa = x.clone().to(dev, dtype).requires_grad_(True)
        s = A.AudioSignal(xa, 44100)
        if dtype == torch.float64:
            s.audio_data = xa                      # (the constructor casts float64 input to float32)
        X = s.stft(**kw)
        name = type(X.grad_fn).__name__
        wts = torch.randn(X.shape, generator=torch.Generator().manual_seed(5)).to(dev, dtype)
        loss = (X.abs() * wts).sum() + (X.abs().clamp(1e-5).log10() * wts).mean() + (X.real * wts + X.imag * wts.flip(-1)).sum()
        (gx,) = torch.autograd.grad(loss, xa)
        return float(loss), gx, name, tuple(X.shape)

    l_ref, g_ref, _, shp_ref = loss_and_grad("cpu", torch.float64)
    l_got, g_got, name, shp = loss_and_grad("cuda", torch.float32)
    assert shp == shp_ref
    assert name in ("_NativeStftGeneralBackward", "_NativeStftBackward"), name        # not torch.stft's backward
    assert abs(l_got - l_ref) <= 1e-4 * abs(l_ref)
    assert rel_err(g_got.double(), g_ref) < REL, rel_err(g_got.double(), g_ref)


def test_mel_autograd_general_sizes():
    """mel_spectrogram under autograd at a run-time size and with match_stride: the STFT below the (torch) magnitude and
    basis product is the native pair, the gradient matches float64."""
    x = synth.audio_batch(2, 1, 16000, seed=77, gaps=False)
    for kw in (dict(window_length=1200, hop_length=300), dict(window_length=2048, hop_length=512, match_stride=True)):
        def run(dev, dtype):
            xa = x.clone().to(dev, dtype).requires_grad_(True)
            s = A.AudioSignal(xa, 24000)
            if dtype == torch.float64:
                s.audio_data = xa
            if dtype == torch.float64:             # (the float32 basis does not multiply a float64 magnitude: by hand)
                X = s.stft(**kw)
                basis = torch.from_numpy(s.get_mel_filters(24000, kw["window_length"], 40)).double()
                mel = (X.abs().transpose(2, -1) @ basis.T).transpose(-1, 2)
            else:
                mel = s.mel_spectrogram(40, **kw)
            loss = mel.clamp(1e-5).log10().mean() + mel.sum() * 1e-3
            (gx,) = torch.autograd.grad(loss, xa)
            return gx, type(s.stft_data.grad_fn).__name__
        g_ref, _ = run("cpu", torch.float64)
        g_got, name = run("cuda", torch.float32)
        assert "Native" in name, name
        assert rel_err(g_got.double(), g_ref) < REL, (kw, rel_err(g_got.double(), g_ref))


def test_stft_mel_into_caller_buffers():
    """kernels.stft_mel(out=(stft_buf, mel_buf)): the same numbers into caller-provided buffers (fused and tiled sizes);
    a buffer of the wrong shape is refused."""
    from audiotools_amd import kernels, tables
    x = synth.audio_batch(3, 2, 30000, seed=11, gaps=False).cuda()
    for n_fft, hop, sr in ((2048, 512, 44100), (512, 128, 16000), (4096, 1024, 96000)):
        win = tables.window("hann", n_fft, x.device)
        mel = (tables.mel_units(sr, n_fft, 40, 0.0, None, x.device) + (40,)) if kernels.stft_fused_supported(n_fft) else \
            (tables.mel_bands(sr, n_fft, 40, 0.0, None, x.device) + (40,))
        X0, M0 = kernels.stft_mel(x, win, n_fft, hop, mel=mel)
        N, F = X0.shape[-1], X0.shape[-2]
        sb = torch.full((3, 2, N, F), float("nan"), dtype=torch.complex64, device="cuda")
        mb = torch.full((3, 2, N, 40), float("nan"), device="cuda")
        X1, M1 = kernels.stft_mel(x, win, n_fft, hop, mel=mel, out=(sb, mb))
        assert X1.data_ptr() == sb.data_ptr() and M1.data_ptr() == mb.data_ptr()
        assert torch.equal(X0, X1) and torch.equal(M0, M1)
        with pytest.raises(ValueError):
            kernels.stft_mel(x, win, n_fft, hop, mel=mel, out=(sb[:, :, :-1], mb))


def test_placement_aware_output_pool_semantics():
    """kernels._PlacedOutputs (round 5): large STFT outputs come from a small pool of buffer sets chosen by timing the real
    kernel at the first call of a shape.  The semantics stay those of a fresh allocation: a result is never overwritten while
    ANY tensor references its storage (views, stft_data of a signal, saved autograd tensors), a released buffer is reused,
    more simultaneous results than the pool holds fall back to plain allocations, and the numbers do not depend on the pool."""
    from audiotools_amd import kernels, tables
    assert kernels._PlacedOutputs.enabled is False and kernels.output_placement() == [], "the pool is an opt-in (round 6)"
    # a small threshold so that a test-sized batch takes the pool; three buffers per shape; calibration at the first call
    kernels.output_placement(enabled=True, min_bytes=1 << 20, keep=3, calibrate_after=1)
    try:
        x = synth.audio_batch(8, 2, 88200, seed=21, gaps=False).cuda()
        win = tables.window("hann", 2048, x.device)
        mel = tables.mel_units(44100, 2048, 80, 0.0, None, x.device) + (80,)
        kernels.output_placement(enabled=False)
        Xref, Mref = kernels.stft_mel(x, win, 2048, 512, mel=mel)
        kernels.output_placement(enabled=True)
        X1, M1 = kernels.stft_mel(x, win, 2048, 512, mel=mel)                  # calibration: CANDIDATES sets timed, KEEP kept
        rep = kernels.output_placement()
        assert len(rep) == 1 and len(rep[0]["calibration_ms"]) == kernels._PlacedOutputs.CANDIDATES and len(rep[0]["kept_ms"]) == 3
        assert rep[0]["kept_ms"] == sorted(rep[0]["calibration_ms"])[:3]
        assert torch.equal(X1, Xref) and torch.equal(M1, Mref)
        held = [(X1, M1)]
        ptrs = {X1.data_ptr()}
        for _ in range(4):                                                     # five results alive at once: three pooled, two plain
            X, M = kernels.stft_mel(x * 0.5, win, 2048, 512, mel=mel)
            assert X.data_ptr() not in ptrs
            ptrs.add(X.data_ptr())
            held.append((X, M))
        assert torch.equal(held[0][0], Xref) and torch.equal(held[0][1], Mref)  # the first result is untouched
        assert torch.equal(held[1][0], held[4][0])
        p_first = held[0][0].data_ptr()
        view_only = torch.view_as_real(held[0][0])                             # a VIEW keeps the storage alive ...
        del held[0]
        del X1, M1
        Xn, _ = kernels.stft_mel(x * 0.25, win, 2048, 512, mel=mel)
        assert Xn.data_ptr() != p_first and torch.equal(torch.view_as_complex(view_only), Xref)
        del view_only, Xn                                                      # ... and once it is gone the pooled set is handed out again
        pooled = {kernels.stft_mel(x, win, 2048, 512, mel=mel)[0].data_ptr() for _ in range(3)}
        assert len(pooled) == 1                                                # released at once, reused at once: one (the fastest free) set
        # a signal keeps its stft_data: two results alternate, both from the pool, neither overwritten while it is stft_data
        sig = A.AudioSignal(x, 44100)
        m_a = sig.mel_spectrogram(80).clone()
        s_a = sig.stft_data
        m_b = sig.mel_spectrogram(80)
        assert sig.stft_data.data_ptr() != s_a.data_ptr() and torch.equal(s_a, Xref) and torch.equal(m_a, m_b)
        # ... and a signal nobody else looks into gets the SAME (fastest free) spectrum buffer call after call: stft() /
        # mel_spectrogram() release the spectrum they are about to replace before the kernel runs
        del s_a, m_b
        sig2 = A.AudioSignal(x, 44100)
        sig2.mel_spectrogram(80)
        p2 = sig2.stft_data.data_ptr()
        for _ in range(3):
            m2 = sig2.mel_spectrogram(80)
            assert sig2.stft_data.data_ptr() == p2 and torch.equal(sig2.stft_data, Xref) and torch.equal(m2, Mref)
        with pytest.warns(UserWarning, match="stft_data changed shape"):       # the reference's warning survives the early release
            sig2.stft(512, 128)
        # the inverse takes its signal buffer from the same pool (its own key): same numbers, nothing overwritten while held
        kernels._placed_outputs.shapes.clear()
        kernels.output_placement(enabled=False)
        y_ref = kernels.istft(Xref, win, 2048, 512, x.shape[-1])
        kernels.output_placement(enabled=True)
        y1 = kernels.istft(Xref, win, 2048, 512, x.shape[-1])
        rep = kernels.output_placement()
        assert [r["op"] for r in rep] == ["istft"] and len(rep[0]["calibration_ms"]) == kernels._PlacedOutputs.CANDIDATES
        y2 = kernels.istft(Xref * 0.5, win, 2048, 512, x.shape[-1])
        assert y2.data_ptr() != y1.data_ptr()
        assert torch.equal(y1, y_ref), float((y1 - y_ref).abs().max())
        assert torch.allclose(y2, 0.5 * y_ref, atol=1e-6), float((y2 - 0.5 * y_ref).abs().max())
        p1 = y1.data_ptr()
        del y1
        assert kernels.istft(Xref, win, 2048, 512, x.shape[-1]).data_ptr() == p1
    finally:
        kernels.output_placement(enabled=False, min_bytes=256 << 20, keep=1, calibrate_after=3)
        kernels._placed_outputs.calibrations = 0


def test_placement_pool_is_a_good_citizen():
    """VERDICT r05 #6 / ADVICE r05: the pool is off by default; opted in, it calibrates at the third call of a shape, inside
    FREE_FRACTION of the memory that is free at that moment; afterwards it pins KEEP = 1 buffer, the losing candidates are
    torch's to reuse -- an allocation as large as everything that is still free succeeds on a nearly full device --, and
    release_workspaces() returns the pinned bytes."""
    from audiotools_amd import kernels, tables
    dev = torch.device("cuda")
    x = synth.audio_batch(16, 2, 4 * 44100, seed=3, gaps=False).cuda()
    win = tables.window("hann", 2048, dev)
    N = 1 + x.shape[-1] // 512
    nbytes = 16 * 2 * N * 1025 * 8                                    # 90 MB of spectrum
    Xref, _ = kernels.stft_mel(x, win, 2048, 512)
    assert kernels.output_placement() == [] and kernels._placed_outputs.bytes_held() == 0
    torch.cuda.empty_cache()
    free_b, _total = torch.cuda.mem_get_info(dev)
    # a nearly full device: ten spectra of room.  The room is MEASURED: the driver's free figure does not fall by exactly the
    # size of a 290 GB allocation (0.5 GB less on some boxes: sixteen spectra of room instead of ten), so the bulk goes first
    # with 2 GiB to spare and a second allocation takes what the free figure then shows beyond ten spectra
    blocker = [torch.empty(free_b - 10 * nbytes - (2 << 30), dtype=torch.uint8, device=dev)]
    try:
        blocker.append(torch.empty(torch.cuda.mem_get_info(dev)[0] - 10 * nbytes, dtype=torch.uint8, device=dev))
        assert 9.5 * nbytes <= torch.cuda.mem_get_info(dev)[0] <= 10.5 * nbytes
        kernels.output_placement(enabled=True, min_bytes=1 << 20)
        kernels._placed_outputs.calibrations = 0
        for call in range(2):
            X, _ = kernels.stft_mel(x, win, 2048, 512)
            assert kernels.output_placement() == [], "no calibration before the third call of a shape"
            del X
        X, _ = kernels.stft_mel(x, win, 2048, 512)
        rep = kernels.output_placement()
        assert len(rep) == 1 and 2 <= len(rep[0]["calibration_ms"]) <= 5, rep         # half of what was free, not all of it
        assert len(rep[0]["kept_ms"]) == 1 and rep[0]["bytes_held"] == nbytes == kernels._placed_outputs.bytes_held()
        assert torch.equal(X, Xref)
        p = X.data_ptr()
        del X
        big = torch.empty(7 * nbytes, dtype=torch.uint8, device=dev)    # everything but the pinned buffer (and a margin) is still available
        X2, _ = kernels.stft_mel(x, win, 2048, 512)
        assert X2.data_ptr() == p and torch.equal(X2, Xref)
        del big, X2
        assert kernels.release_workspaces() == nbytes and kernels._placed_outputs.bytes_held() == 0
    finally:
        del blocker
        kernels.output_placement(enabled=False, min_bytes=256 << 20, keep=1, calibrate_after=3)
        kernels._placed_outputs.calibrations = 0
        torch.cuda.empty_cache()


def test_c_abi_error_codes_and_degenerate_inputs():
    """The C ABI never throws: 0 = ok, -1 = bad argument, -2 = no kernel for the request; empty
    batches are no-ops; the Python layer turns codes into NativeError / the reference's errors."""
    import ctypes
    from audiotools_amd import _native, kernels, tables
    lib = _native.lib()
    dev = torch.device("cuda")
    st = _native.current_stream(dev)
    x = torch.zeros(2, 1, 4096, device=dev)
    win = tables.window("hann", 512, dev)
    tw = tables.stft_twiddles(512, dev)
    out = torch.empty(2, 1, 33, 257, dtype=torch.complex64, device=dev)
    p = _native.ptr
    args = lambda **k: [k.get("x", p(x)), k.get("rows", 2), k.get("T", 4096), p(win), p(tw), k.get("n_fft", 512),
                        k.get("hop", 128), 0, 0, 0, 0, k.get("n_out", 33), k.get("out", p(out)), None, None, 0, 0, None, st]
    assert lib.at_stft_mel_f32(*args()) == 0
    assert lib.at_stft_mel_f32(*args(rows=0)) == 0                      # empty batch
    assert lib.at_stft_mel_f32(*args(x=None)) == -1
    assert lib.at_stft_mel_f32(*args(out=None)) == -1                   # stft_data is always produced
    assert lib.at_stft_mel_f32(*args(hop=0)) == -1
    assert lib.at_stft_mel_f32(*args(n_out=34)) == -1                   # more frames than the signal has
    assert lib.at_stft_mel_f32(*args(T=200)) == -1                      # reflect padding needs n_fft/2 < T
    assert lib.at_stft_mel_f32(*args(n_fft=502)) == -2                  # n_fft / 2 = 251 is prime: no kernel
    assert lib.at_stft_mel_f32(*args(n_fft=501)) == -2                  # odd
    assert lib.at_stft_mel_f32(*args(n_fft=32768)) == -2                # longer than any kernel
    assert lib.at_stft_mel_f32(*args(n_fft=500)) == 0                   # 2 * 2 * 5^3: the generic mixed-radix kernel
    assert lib.at_lufs_f32(None, 1, 1, 100, None, None, 2, 4, 1, 1.0, -70.0, 0, None, None, 0, st) == -1
    assert lib.at_fir_fft_f32(p(x), 2, 1, 4096, p(win), 1, 512, 255, 0, None, p(x), st) == -1      # x aliases out / no twiddles
    assert lib.at_istft_workspace_bytes(2, 0, 512, 128) == -1
    assert lib.at_resample_f32(p(x), 2, 4096, p(win), None, 3, 2, 10, 1, 4, p(x), 10, st) == -1
    assert lib.at_fftconv_circ_f32(p(x), p(x), None, 2, 1, 3, 4096, p(x), None, 0, st) == -1     # Cir must be 1 or C
    torch.cuda.synchronize()
    # Python layer
    with pytest.raises(_native.NativeError):
        _native.check(-2, "at_stft_mel_f32")
    with pytest.raises(_native.NativeError):
        kernels.stft_mel(torch.zeros(1, 1, 4096), win.cpu(), 512, 128)   # CPU tensor handed to a native launcher
    e = A.AudioSignal(torch.zeros(0, 1, 4096), 16000).to("cuda")          # empty batch through the object API
    assert e.stft(512, 128).shape == (0, 1, 257, 33)
    one = A.AudioSignal(torch.randn(1, 1, 300), 16000, stft_params=A.STFTParams(512, 128)).to("cuda")
    assert one.stft().shape == (1, 1, 257, 3)                              # shortest legal signal class (T > n_fft/2)
    assert one.loudness().shape == (1,)                                    # < 0.5 s is zero-padded, not an error
    with pytest.raises(AssertionError):
        A.AudioSignal(torch.randn(1, 1, 4096), 16000).to("cuda").stft(512, 100, match_stride=True)


@pytest.mark.parametrize("name", ["ClippingDistortion", "Equalizer", "Quantization", "MuLawQuantization", "NoiseFloor",
                                  "VolumeChange", "VolumeNorm", "Silence", "LowPass", "HighPass", "RescaleAudio",
                                  "ShiftPhase", "InvertPhase", "FrequencyMask", "TimeMask", "MaskLowMagnitudes",
                                  "Smoothing", "Identity", "SpectralDenoising"])
def test_transforms_gpu_vs_cpu(name):
    """Every loader-free transform of data/transforms.py with the same instantiated parameters on
    the HIP path and on the CPU path (which tests/test_transforms.py pins seed-for-seed to the
    unmodified reference), batch of 4, half of the items masked out (prob 0.5)."""
    from audiotools_amd import transforms as tfm
    x = synth.audio_batch(4, 1, 22050, seed=17, gaps=False)
    t = getattr(tfm, name)(prob=0.5) if name != "Identity" else tfm.Identity()
    sig = A.AudioSignal(x.clone(), 44100)
    kw = t.batch_instantiate([3, 4, 5, 6], sig)
    ref = t(sig.clone(), **kw).audio_data
    got = t(sig.clone().to("cuda"), **A.util.prepare_batch(kw, "cuda")).audio_data
    if name in ("MaskLowMagnitudes", "SpectralDenoising"):   # threshold on a float32 log: allow isolated bin flips
        assert float(((got.cpu() - ref).abs() > 1e-3 * ref.abs().max()).float().mean()) < 1e-3
    else:
        assert rel_err(got, ref) < REL, name


def test_transform_chain_gpu_vs_cpu():
    """cfg4-style Compose (per-item LowPass cutoffs, Equalizer, RoomImpulseResponse from a tensor
    bank with DRR + EQ, VolumeNorm, spectral masks) end to end: HIP path vs CPU path."""
    from audiotools_amd import transforms as tfm
    B, T, SR = 6, 24000, 16000
    x = synth.audio_batch(B, 1, T, seed=23, gaps=False, sample_rate=SR)
    g = torch.Generator().manual_seed(9)
    bank = torch.randn(5, 1, 4000, generator=g) * torch.exp(-torch.arange(4000) / 600.0)
    chain = tfm.Compose(tfm.LowPass(cutoff=("choice", [2000, 4000, 6000])), tfm.Equalizer(n_bands=6),
                        tfm.RoomImpulseResponse(loader=tfm.TensorLoader(bank, SR), duration=0.25),
                        tfm.VolumeNorm(("uniform", -30, -20)), tfm.FrequencyMask(), tfm.TimeMask(), tfm.ShiftPhase())
    sig = A.AudioSignal(x.clone(), SR)
    kw = chain.batch_instantiate(list(range(B)), sig)
    ref = chain(sig.clone(), **kw).audio_data
    got = chain(sig.clone().to("cuda"), **A.util.prepare_batch(kw, "cuda")).audio_data
    assert rel_err(got, ref) < 5 * REL     # seven stages: the per-stage 1e-4 budget accumulates


def test_device_stager_overlapped_copies():
    """Pinned-host -> device staging on a side stream: every batch arrives intact and in order while
    the consumer keeps the previous one busy (depth 2 and 3, more batches than buffers)."""
    from audiotools_amd.data import DeviceStager
    g = torch.Generator().manual_seed(1)
    batches = [torch.randn(4, 2, 44100, generator=g) for _ in range(7)]
    for depth in (2, 3):
        sums = []
        for x in DeviceStager(batches, "cuda", depth=depth):
            assert x.is_cuda
            s = A.AudioSignal(x, 44100)
            sums.append((s.mel_spectrogram(80).sum() + s.loudness().sum()).clone())   # real work on the buffer
        ref = [A.AudioSignal(b.cuda(), 44100) for b in batches]
        ref = [r.mel_spectrogram(80).sum() + r.loudness().sum() for r in ref]
        assert torch.allclose(torch.stack(sums), torch.stack(ref), rtol=1e-5)


@pytest.mark.parametrize("win,n_mels,T", [(2048, 80, 22050 + 7), (512, 80, 16000), (1024, 64, 12001), (256, 40, 5000), (64, 10, 1000)])
def test_mel_autograd_fused_backward(win, n_mels, T):
    """Log-mel loss (metrics/spectral.py MelSpectrogramLoss) through the fused forward kernel and
    at_stft_mel_adjoint_f32 (dL/dX never materialised) vs torch autograd of the reference
    formulation on CPU; also the mixed case where stft_data is used as well (torch-composed
    spectrum gradient + native adjoint)."""
    x = synth.audio_batch(2, 2, T, seed=win + n_mels, gaps=False)

    def grads(dev, use_X):
        xa = x.clone().to(dev).requires_grad_(True)
        s = A.AudioSignal(xa, 44100)
        mel = s.mel_spectrogram(n_mels, window_length=win, hop_length=win // 4, window_type="hann")
        wts = torch.randn(mel.shape, generator=torch.Generator().manual_seed(7)).to(dev)
        loss = (mel.clamp(1e-5).log10() * wts).sum() + (mel * wts).mean()
        if use_X:
            loss = loss + s.stft_data.abs().pow(2).mean()
        (g,) = torch.autograd.grad(loss, xa)
        return float(loss), g

    for use_X in (False, True):
        l_ref, g_ref = grads("cpu", use_X)
        l_got, g_got = grads("cuda", use_X)
        assert abs(l_got - l_ref) <= 1e-4 * abs(l_ref)
        assert rel_err(g_got, g_ref) < REL, use_X


@pytest.mark.parametrize("config", ["north_star", "cfg4", "cfg5"])
def test_bench_multi_rank_control_flow_on_one_device(config):
    """bench.py with TWO ranks sharing cuda:0 over gloo (`--shared-device`, a test-only switch: RCCL refuses two ranks on one
    GPU): every rank must enter the same collectives in the same order -- table broadcasts, the timed regions' barriers and
    reductions, the all-reduced parity verdict, the collective plain-allocation pass, the closing barrier -- or the run hangs,
    which on the driver's 8-GPU node would be the first time anybody saw it."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    batch = {"north_star": 40, "cfg4": 16, "cfg5": 8}[config]      # (north star: 20 items per rank = a 282 MB spectrum, so the output pool calibrates on both ranks)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--shared-device", "--config", config,
                          "--batch", str(batch), "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["world_size"] == 2 and d["backend"] == "gloo" and d["parity_check"]["ok"] is True
    assert len(d["per_rank_ms_per_step"]) == 2 and d["config"]["items_per_gpu"] * 2 == batch
    if config == "north_star":
        assert d["parity_check"]["every_rank_device_check"]["ok_all_ranks"] is True
        assert d["roofline"]["placement"]["kernel_ms_plain_allocation"] > 0


def test_backward_pass_as_the_first_gpu_work_of_a_process():
    """Round 6 (sessions s05 / s06): the inverse transform's adjoint built its overlap-add envelope with conv_transpose1d -- a
    MIOpen call -- and the FIRST MIOpen call of a process made from autograd's worker thread aborts the interpreter on this
    stack.  It only showed when no forward convolution had run before (a test selection; a training script whose first step
    is a spectral loss).  The adjoints are MIOpen-free now; this runs one in a fresh process, as its first GPU work."""
    import subprocess
    import sys

    code = (
        "import sys, torch; sys.path.insert(0, %r)\n"
        "import audiotools_amd as A\n"
        "X = torch.randn(2, 2, 1025, 40, dtype=torch.complex64, device='cuda', requires_grad=True)\n"
        "s = A.AudioSignal(torch.zeros(2, 2, 40 * 512 - 100), 44100).to('cuda')\n"
        "s.stft_data = X\n"
        "y = s.istft(2048, 512, 'hann', False, length=40 * 512 - 100).audio_data\n"
        "(g,) = torch.autograd.grad((y ** 2).mean(), X)\n"
        "x = torch.randn(2, 2, 30000, device='cuda', requires_grad=True)\n"
        "m = A.AudioSignal(x, 44100).mel_spectrogram(80)\n"
        "(gx,) = torch.autograd.grad(m.sum(), x)\n"
        "torch.cuda.synchronize(); assert torch.isfinite(g).all() and torch.isfinite(gx).all(); print('ok')\n"
    ) % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stderr[-1500:])


@pytest.mark.parametrize("win,hop,nfr,T", [(2048, 512, 40, 40 * 512 - 100), (512, 128, 60, 59 * 128), (1024, 512, 21, 10007),
                                            (256, 32, 90, 89 * 32 + 5), (64, 4, 120, 470)])
def test_istft_autograd_native(win, hop, nfr, T):
    """Gradients through the native istft() (fused inverse kernel forward, forward-STFT kernel as its
    adjoint) equal torch.istft's on CPU, for spectra that are NOT the STFT of a signal."""
    g = torch.Generator().manual_seed(win + hop)
    Xr = torch.randn(2, 2, win // 2 + 1, nfr, 2, generator=g)
    wts = torch.randn(2, 2, T, generator=g)

    def run(dev):
        X = torch.view_as_complex(Xr.clone()).to(dev).requires_grad_(True)
        s = A.AudioSignal(torch.zeros(2, 2, T), 44100).to(dev)
        s.stft_data = X
        y = s.istft(win, hop, "hann", False, length=T).audio_data
        loss = (y * wts.to(dev)).sum() + (y ** 2).mean()
        (gx,) = torch.autograd.grad(loss, X)
        return y.detach(), gx

    y_ref, g_ref = run("cpu")
    y_got, g_got = run("cuda")
    assert rel_err(y_got, y_ref) < REL
    assert rel_err(torch.view_as_real(g_got), torch.view_as_real(g_ref)) < REL


@pytest.mark.parametrize("name,kw", [
    ("MultiScaleSTFTLoss", {}),
    ("MelSpectrogramLoss", {}),
    ("MelSpectrogramLoss", {"n_mels": [5, 10, 20, 40, 80, 160, 320], "window_lengths": [32, 64, 128, 256, 512, 1024, 2048],
                            "mel_fmin": [0] * 7, "mel_fmax": [None] * 7, "pow": 1.0, "mag_weight": 0.0}),
    ("PhaseLoss", {})])
def test_training_losses_gpu_vs_cpu(name, kw):
    """metrics/spectral.py losses with the native forward + adjoint kernels (HIP) against the torch
    formulation on CPU (pinned to the unmodified reference by tests/test_metrics.py): value and
    gradient w.r.t. the estimate."""
    from audiotools_amd import metrics
    x = synth.audio_batch(2, 1, 16000, seed=3, gaps=False)
    y = synth.audio_batch(2, 1, 16000, seed=4, gaps=False)
    loss = getattr(metrics.spectral, name)(**kw)

    def run(dev):
        xa = x.clone().to(dev).requires_grad_(True)
        val = loss(A.AudioSignal(xa, 44100), A.AudioSignal(y.clone().to(dev), 44100))
        (g,) = torch.autograd.grad(val, xa)
        return float(val), g

    v_ref, g_ref = run("cpu")
    v_got, g_got = run("cuda")
    # PhaseLoss wraps phase differences discontinuously and differentiates angle(): ill-conditioned
    # where |X| ~ 0 or the difference sits at +-pi; compare loosely and in the mean
    assert abs(v_got - v_ref) <= (1e-2 if name == "PhaseLoss" else 1e-4) * abs(v_ref) + 1e-6
    if name == "PhaseLoss":
        assert float((g_got.cpu() - g_ref).abs().mean() / g_ref.abs().mean()) < 1e-2
    else:
        assert rel_err(g_got, g_ref) < REL


# ----------------------------------------------------------------------------- istft
@pytest.mark.parametrize("win,hop,wt,ms", [(2048, 512, "hann", False), (2048, 512, "sqrt_hann", True),
                                           (512, 128, "sqrt_hann", False), (512, 128, "hann", True),
                                           (1024, 256, "hann", False), (256, 64, "sqrt_hann", True),
                                           (512, 100, "hann", False), (64, 16, "hann", False),
                                           (1024, 512, "hann", False), (512, 64, "hann", False),
                                           (128, 8, "sqrt_hann", False), (32, 8, "hann", True)])
def test_istft_vs_oracle_and_roundtrip(win, hop, wt, ms):
    """tests/core/test_audio_signal.py:400-456: istft(stft(x)) == x; plus values vs torch.istft on CPU."""
    x = synth.audio_batch(3, 2, 22050 + 7, seed=win + hop, gaps=False)
    s = A.AudioSignal(x.clone(), 44100).to("cuda")
    X = s.stft(win, hop, wt, ms)
    ref = restate.istft(X.cpu(), win, hop, wt, ms, x.shape[-1])
    y = s.istft(win, hop, wt, ms).audio_data
    assert y.shape == ref.shape
    assert rel_err(y, ref) < REL
    if hop * 4 == win:
        # match_stride drops the two edge frames on each side: only the interior reconstructs
        # (tests/core/test_audio_signal.py:447-456)
        sl = slice(win, -win) if ms else slice(None)
        assert float((y.cpu() - x)[..., sl].abs().max()) < 1e-5


def test_istft_golden_and_modified_spectrum():
    d = np.load(os.path.join(G, "stft_cfg1.npz"))
    s = A.AudioSignal(torch.from_numpy(d["x"]), 16000).to("cuda")
    s.stft(512, 128, "hann")
    assert rel_err(s.clone().istft(512, 128, "hann").audio_data, torch.from_numpy(d["istft"])) < REL
    # a spectrum that is NOT the STFT of a signal (time mask + phase shift) still inverts like torch.istft
    x = synth.audio_batch(2, 1, 16000, seed=9, gaps=False)
    g = A.AudioSignal(x.clone(), 16000).to("cuda")
    g.stft()
    g.mask_timesteps(0.2, 0.4).shift_phase(0.3)
    ref = restate.istft(g.stft_data.cpu(), 512, 128, "hann", False, 16000)
    assert rel_err(g.istft().audio_data, ref) < REL
    with pytest.raises(RuntimeError):
        A.AudioSignal(x.clone(), 16000).to("cuda").istft()


# ------------------------------------------------------ BASELINE.json full-size configurations
def _device_batch(B, C, T, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = (0.1 * torch.randn(B, C, T, device="cuda", generator=g)).clamp_(-1, 1)
    x *= (10 ** (-30 * torch.rand(B, device="cuda", generator=g) / 20))[:, None, None]
    return x


def test_cfg2_full_size_stft_mel():
    """configs[1]: batch 256 x 2ch x 10s @44.1k, STFT(2048/512) + 80-bin mel.  Oracle on a
    subset of the items (rows are independent), linearity and finiteness on all of them."""
    B, C, T = 256, 2, 441000
    x = _device_batch(B, C, T, 11)
    s = A.AudioSignal(x, 44100)
    mel = s.mel_spectrogram(80)
    assert mel.shape == (B, C, 80, 862) and s.stft_data.shape == (B, C, 1025, 862)
    assert torch.isfinite(mel).all()
    idx = [0, 37, 255]
    xs = x[idx].cpu()
    Xr = restate.stft(xs, 2048, 512)
    assert rel_err(s.stft_data[idx], Xr) < REL
    assert rel_err(mel[idx], restate.mel_spectrogram(Xr, 44100, 80)) < REL
    # mel is linear in |X| and |X| is homogeneous: scaling the audio scales the mel
    mel2 = A.AudioSignal(0.5 * x, 44100).mel_spectrogram(80)
    assert rel_err(mel2, 0.5 * mel) < REL
    # every frame of every row was written: a checksum over frames matches a second run
    mel3 = A.AudioSignal(x, 44100).mel_spectrogram(80)
    assert torch.equal(mel3, mel)


def test_north_star_full_size():
    """BASELINE.json `metric` at its own size, as ONE launch each: batch 512 x 2ch x 10 s @44.1 kHz mel_spectrogram(80)
    [fused STFT 2048/512 + mel] + loudness() -- the persistent grid's schedule (runs per wave, XCD spans) depends on the row
    count, so the B = 256 test above does not cover the benchmarked launch.  Oracle on items {0, 37, 255, 511}, per row."""
    B, C, T = 512, 2, 441000
    x = _device_batch(B, C, T, 41)
    for i in range(0, B, 20):
        x[i, :, 3 * 44100: 5 * 44100] = 0          # bench.py's 5 % of items with 2 s of digital silence
    s = A.AudioSignal(x, 44100)
    mel = s.mel_spectrogram(80)
    l = s.loudness()
    assert mel.shape == (B, C, 80, 862) and s.stft_data.shape == (B, C, 1025, 862) and l.shape == (B,)
    assert torch.isfinite(mel).all() and torch.isfinite(l).all()
    idx = [0, 37, 255, 511]
    xs = x[idx].cpu()
    Xr = restate.stft(xs, 2048, 512)
    assert rel_err(s.stft_data[idx], Xr) < REL
    assert rel_err(mel[idx], restate.mel_spectrogram(Xr, 44100, 80)) < REL
    assert float((l[idx].cpu() - restate.loudness(xs, 44100)).abs().max()) < LU
    # every frame of every row: the same launch twice is bit-equal, and the 256-item launch agrees on its items
    mel2 = A.AudioSignal(x, 44100).mel_spectrogram(80)
    assert torch.equal(mel2, mel)
    half = A.AudioSignal(x[:256], 44100)
    assert rel_err(half.mel_spectrogram(80), mel[:256].cpu()) < 1e-6          # (another schedule of the same frames)
    assert float((half.loudness() - l[:256]).abs().max()) < 1e-4


def test_cfg3_full_size_loudness():
    """configs[2]: batch 512 x 2ch x 10s @44.1k LUFS.  Oracle on a subset, gain property on all,
    permutation invariance (items are independent), silence clamp."""
    B, C, T = 512, 2, 441000
    x = _device_batch(B, C, T, 12)
    x[5] = 0.0
    x[9, :, : 6 * 44100] = 0.0            # long digital-silence gap: absolute gate
    l = A.AudioSignal(x, 44100).loudness()
    assert l.shape == (B,) and float(l[5]) == -70.0
    idx = [0, 9, 200, 511]
    ref = restate.loudness(x[idx].cpu(), 44100)
    assert float((l[idx].cpu() - ref).abs().max()) < LU
    l6 = A.AudioSignal(0.5 * x, 44100).loudness()
    keep = l > -60
    assert float(((l6 - l)[keep] + 6.0206).abs().max()) < 1e-2
    perm = torch.randperm(B, device="cuda")
    lp = A.AudioSignal(x[perm], 44100).loudness()
    assert float((lp - l[perm]).abs().max()) < 1e-4


# ------------------------------------------------------ round 2: rows the review found untested
@pytest.mark.parametrize("B,C,T", [(1, 1, 4096), (1, 1, 4098), (3, 2, 44100), (5, 1, 6144), (2, 2, 100000), (64, 1, 8192)])
@pytest.mark.parametrize("wt", ["hann", "sqrt_hann"])
def test_stft_default_params_kernel_shapes(B, C, T, wt):
    """n_fft 2048 / hop 512 (the reference's defaults at 44.1 kHz) takes the specialised kernel
    (paired last pass, csrc/stft.hip stft_mel_kernel_v2): short rows, one row, run boundaries, with
    and without the fused mel."""
    x = synth.audio_batch(B, C, T, seed=T + B, gaps=False)
    s = A.AudioSignal(x.clone(), 44100).to("cuda")
    ref = restate.stft(x, 2048, 512, wt)
    assert rel_err(s.stft(2048, 512, wt), ref) < REL
    mel = s.mel_spectrogram(80, window_type=wt)
    assert rel_err(mel, restate.mel_spectrogram(ref, 44100, 80)) < REL
    assert rel_err(s.stft_data, ref) < REL


def test_magnitude_phase_log_magnitude_gpu():
    """a9 (audio_signal.py:1428-1516) on the device vs the oracle: getters, setters, log_magnitude."""
    x = synth.audio_batch(3, 2, 30000, seed=4, gaps=False)
    s = A.AudioSignal(x.clone(), 44100).to("cuda")
    X = restate.stft(x, 2048, 512)
    assert rel_err(s.magnitude, X.abs()) < REL
    # the phase of a bin is meaningful relative to its magnitude: compare mag * e^{i phase}
    assert rel_err(s.magnitude * torch.exp(1j * s.phase), X) < REL
    for kw in ({}, {"ref_value": 0.5, "top_db": 40.0}, {"top_db": None, "amin": 1e-3}):
        got, ref = s.log_magnitude(**kw).cpu(), restate.log_magnitude(X, **kw)
        assert float((got - ref).abs().max()) < 2e-3, kw          # dB; 1e-4 relative on |X| = 8.7e-4 dB
    g = torch.Generator().manual_seed(0)
    mag = torch.rand(X.shape, generator=g)
    ph0 = s.phase.cpu()       # the phase of a near-zero bin is ill-conditioned: use the device's own
    s.magnitude = mag.cuda()
    assert rel_err(s.stft_data, mag * torch.exp(1j * ph0)) < REL
    ph = (torch.rand(X.shape, generator=g) - 0.5) * 6
    s.phase = ph.cuda()
    assert rel_err(s.stft_data, mag * torch.exp(1j * ph)) < REL


@pytest.mark.parametrize("eq", [False, True])
def test_mix_gpu_vs_oracle(eq):
    sr = 44100
    x = synth.audio_batch(4, 2, 60000, seed=5, gaps=False)
    o = synth.audio_batch(4, 2, 45000, seed=6, gaps=False)
    snr = torch.tensor([0.0, 5.0, 10.0, 20.0])
    eq_v = -torch.rand(4, 3, generator=torch.Generator().manual_seed(1)) if eq else None
    got = A.AudioSignal(x.clone(), sr).to("cuda").mix(A.AudioSignal(o.clone(), sr).to("cuda"), snr, eq_v).audio_data
    ref = restate.mix(x, o, sr, snr, eq_v)
    assert rel_err(got, ref) < REL


@pytest.mark.parametrize("name", ["BackgroundNoise", "CrossTalk", "RoomImpulseResponse", "GlobalVolumeNorm"])
def test_loader_transforms_gpu_vs_cpu(name):
    """The loader-backed transforms with the same instantiated parameters on the HIP path and on the
    CPU path (tests/test_api_parity.py pins the CPU path seed-for-seed to the unmodified reference)."""
    from audiotools_amd import transforms as tfm
    sr = 44100
    g = torch.Generator().manual_seed(3)
    x = synth.audio_batch(4, 1, 44100, seed=31, gaps=False)
    sig = A.AudioSignal(x.clone(), sr)
    if name == "RoomImpulseResponse":
        bank = torch.randn(5, 1, 30000, generator=g) * torch.exp(-torch.arange(30000) / 4000.0)
        t = tfm.RoomImpulseResponse(loader=tfm.TensorLoader(bank, sr), duration=0.5)
    elif name == "GlobalVolumeNorm":
        t = tfm.GlobalVolumeNorm(db=("uniform", -30, -20))
        sig.metadata["loudness"] = -17.5
    else:
        bank = 0.1 * torch.randn(5, 2, 80000, generator=g)
        t = getattr(tfm, name)(loader=tfm.TensorLoader(bank, sr))
    kw = t.batch_instantiate([3, 4, 5, 6], sig)
    ref = t(sig.clone(), **kw).audio_data
    got = t(sig.clone().to("cuda"), **A.util.prepare_batch(kw, "cuda")).audio_data
    assert rel_err(got, ref) < REL, name


def test_convolve_broadcast_shapes():
    """effects.py:106-111 broadcasts rfft(ir) * rfft(x): one IR for a whole batch, and a stereo IR
    on a mono signal (these failed on the native path only)."""
    g = torch.Generator().manual_seed(2)
    x = 0.1 * torch.randn(3, 2, 20000, generator=g)
    ir = torch.randn(1, 1, 3000, generator=g) * torch.exp(-torch.arange(3000) / 400.0)
    got = A.AudioSignal(x.clone(), 16000).to("cuda").convolve(A.AudioSignal(ir.clone(), 16000).to("cuda")).audio_data
    ref = restate.convolve(x, ir.expand(3, 1, -1))
    assert rel_err(got, ref) < REL
    xm = 0.1 * torch.randn(2, 1, 20000, generator=g)
    ir2 = torch.randn(2, 2, 3000, generator=g) * torch.exp(-torch.arange(3000) / 400.0)
    got = A.AudioSignal(xm.clone(), 16000).to("cuda").convolve(A.AudioSignal(ir2.clone(), 16000).to("cuda"), start_at_max=False)
    ref = A.AudioSignal(xm.clone(), 16000).convolve(A.AudioSignal(ir2.clone(), 16000), start_at_max=False)
    assert got.audio_data.shape == (2, 2, 20000) and rel_err(got.audio_data, ref.audio_data) < REL


def test_absmax_propagates_nan():
    x = torch.randn(3, 2, 5000)
    x[1, 0, 777] = float("nan")
    x[1, 0, 4000] = float("nan")
    v, i = kernels.absmax(x.cuda(), want_index=True)
    rv, ri = x.abs().max(-1).values, x.abs().argmax(-1)
    assert torch.equal(torch.isnan(v.cpu()), torch.isnan(rv)) and int(i[1, 0]) == 777
    ok = ~torch.isnan(rv)
    assert torch.equal(v.cpu()[ok], rv[ok]) and torch.equal(i.cpu()[ok], ri[ok])


def test_resample_unsupported_ratio_falls_back():
    """A gcd-reduced source rate too large for the kernel's LDS tile (44100 -> 16001) takes the torch
    formulation instead of raising."""
    x = synth.audio_batch(1, 1, 9000, seed=8, gaps=False)
    assert not kernels.resample_supported(44100, 16001) and kernels.resample_supported(44100, 16000)
    got = A.AudioSignal(x.clone(), 44100).to("cuda").resample(16001).audio_data
    ref = restate.resample(x, 44100, 16001)
    assert rel_err(got, ref) < REL


def test_mel_loss_gradient_vs_float64():
    """Resolves the round-1 '7-scale grad rel diff 8.8e-4' figure: the multi-scale log-mel loss
    gradient of the native path and of the torch.stft path (both float32 on the GPU) against a
    float64 evaluation of the same formula.  log10(clamp(mel)) has gradients ~1/mel, so float32
    round-off in mel shows up amplified in BOTH float32 paths; the native path must be no worse."""
    from audiotools_amd import metrics, spectral, tables
    wins, mels = [32, 64, 128, 256, 512, 1024, 2048], [5, 10, 20, 40, 80, 160, 320]
    B, C, T, sr = 4, 2, 44100, 44100
    x = synth.audio_batch(B, C, T, seed=1, gaps=False).cuda()
    y = synth.audio_batch(B, C, T, seed=2, gaps=False).cuda()
    loss = metrics.spectral.MelSpectrogramLoss(n_mels=mels, window_lengths=wins, mel_fmin=[0] * 7, mel_fmax=[None] * 7,
                                               pow=1.0, mag_weight=0.0)

    def grad32(native):
        saved = spectral._native_autograd_ok
        if not native:
            spectral._native_autograd_ok = lambda *a: False
        try:
            xa = x.clone().requires_grad_(True)
            loss(A.AudioSignal(xa, sr), A.AudioSignal(y.clone(), sr)).backward()
            return xa.grad.double()
        finally:
            spectral._native_autograd_ok = saved

    def grad64():
        xa = x.double().clone().requires_grad_(True)
        yd = y.double()
        total = 0.0
        for w, m in zip(wins, mels):
            win = torch.from_numpy(tables.window_np("hann", w)).double().cuda()
            basis = torch.from_numpy(tables.mel_filters_np(sr, w, m, 0.0, None)).double().cuda()
            def mel_of(a):
                X = torch.stft(a.reshape(-1, T), w, w // 4, window=win, return_complex=True, center=True)
                return basis @ X.abs()
            lx = mel_of(xa).clamp(1e-5).log10()
            ly = mel_of(yd).clamp(1e-5).log10()
            total = total + (lx - ly).abs().mean()
        total.backward()
        return xa.grad.reshape(B, C, T)

    g64 = grad64()
    scale = g64.abs().max()
    e_native = float((grad32(True) - g64).abs().max() / scale)
    e_torch = float((grad32(False) - g64).abs().max() / scale)
    print(f"7-scale mel-loss gradient vs float64: native {e_native:.2e}, torch.stft float32 {e_torch:.2e}")
    assert e_native < max(2.0 * e_torch, REL)


def _chain_kwargs_cfg4(B, T, SR, seed0):
    from audiotools_amd import transforms as tfm
    g = torch.Generator().manual_seed(77)
    n_ir = 64
    t_ir = torch.arange(2 * SR) / SR
    bank = torch.randn(n_ir, 1, 2 * SR, generator=g) * torch.exp(-t_ir / 0.3)       # randn * exp(-t / 0.3 s)
    chain = tfm.Compose(tfm.LowPass(cutoff=("choice", [4000, 8000, 16000])), tfm.Equalizer(n_bands=6),
                        tfm.RoomImpulseResponse(loader=tfm.TensorLoader(bank, SR), duration=2.0, offset=0.0))
    proto = A.AudioSignal(torch.zeros(B, 1, 8), SR)     # instantiate() only reads rate / channels / batch size
    kw = chain.batch_instantiate([seed0 + i for i in range(B)], proto)
    return chain, kw


def test_cfg4_full_size_chain():
    """configs[3]: batch 1024 x mono x 5 s @48 kHz through Compose(LowPass(choice 4/8/16 kHz) ->
    Equalizer(6 bands) -> RoomImpulseResponse(2 s RIR, DRR U(0,30), EQ)).  Oracle (the restated
    reference ops) on a subset of the items, determinism and permutation equivariance on all rows:
    items are independent, so permuting the batch and its parameters must permute the output."""
    B, T, SR = 1024, 240000, 48000
    chain, kw = _chain_kwargs_cfg4(B, T, SR, 1000)
    x = _device_batch(B, 1, T, 21)
    c = kw["Compose"]
    assert c["2.RoomImpulseResponse"]["ir_signal"].audio_data.shape == (B, 1, 2 * SR)
    idx = [0, 1, 517, 1023]
    ir_subset = c["2.RoomImpulseResponse"]["ir_signal"].audio_data[idx].clone()   # prepare_batch moves signals IN PLACE
    kw_perm_src = _permute_kwargs(kw, torch.arange(B))                            # host copy for the permuted run
    kwd = A.util.prepare_batch(kw, "cuda")
    out = chain(A.AudioSignal(x.clone(), SR), **kwd).audio_data
    assert out.shape == (B, 1, T) and torch.isfinite(out).all()
    xs = x[idx].cpu()
    ref = restate.low_pass(xs, c["0.LowPass"]["cutoff"][idx], SR)
    ref = restate.equalizer(ref, SR, c["1.Equalizer"]["eq"][idx])
    ref = restate.apply_ir(ref, ir_subset, SR, c["2.RoomImpulseResponse"]["drr"][idx], c["2.RoomImpulseResponse"]["eq"][idx])
    assert rel_err(out[idx], ref) < 3 * REL          # three stages of the 1e-4 budget
    # apply_ir restores the peak of ITS input (effects.py:174-177): peak(out) == peak(after EQ)
    mid = A.AudioSignal(x.clone(), SR).low_pass(c["0.LowPass"]["cutoff"].cuda()).equalizer(c["1.Equalizer"]["eq"].cuda())
    assert float((out.abs().amax(-1) / mid.audio_data.abs().amax(-1) - 1).abs().max()) < 1e-4
    # the transform works on a second OBJECT over the impulse responses' samples instead of the reference's clone:
    # the caller's signal keeps its samples and its length
    ir_after = kwd["Compose"]["2.RoomImpulseResponse"]["ir_signal"].audio_data
    assert ir_after.shape == (B, 1, 2 * SR) and torch.equal(ir_after[idx].cpu(), ir_subset)
    out2 = chain(A.AudioSignal(x.clone(), SR), **kwd).audio_data
    assert torch.equal(out2, out)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(0))
    kwp = A.util.prepare_batch(_permute_kwargs(kw_perm_src, perm), "cuda")
    outp = chain(A.AudioSignal(x[perm.cuda()].clone(), SR), **kwp).audio_data
    assert rel_err(outp, out[perm.cuda()]) < 1e-5


def _permute_kwargs(kw, perm):
    out = {}
    for k, v in kw.items():
        if isinstance(v, dict):
            out[k] = _permute_kwargs(v, perm)
        elif hasattr(v, "audio_data"):
            out[k] = A.AudioSignal(v.audio_data[perm].clone(), v.sample_rate)
        elif torch.is_tensor(v) and v.ndim >= 1 and v.shape[0] == perm.numel():
            out[k] = v[perm]
        else:
            out[k] = v
    return out


@pytest.mark.parametrize("B", [256, 2048])
def test_cfg5_full_size_resample_mel(B):
    """configs[4]: one GPU's share of an 8-way shard (256 items) and the WHOLE configuration on one GPU (2048 items: what
    `bench.py --config cfg5` runs; 21.7 GB of input, the resampler's runs of tiles then span several rows per workgroup):
    B x 2ch x 30 s @44.1 kHz -> resample(16000) ->
    mel_spectrogram(80) with the literal (2048, 512) parameters the signal keeps after resample.
    Oracle on a subset of rows, linearity / determinism / finiteness on all of them."""
    C, T = 2, 1323000
    x = _device_batch(B, C, T, 31)
    s = A.AudioSignal(x, 44100)
    s.resample(16000)
    y = s.audio_data
    assert y.shape == (B, C, 480000) and s.sample_rate == 16000 and s.stft_params.window_length == 2048
    mel = s.mel_spectrogram(80)
    assert mel.shape == (B, C, 80, 938) and torch.isfinite(mel).all() and torch.isfinite(y).all()
    idx = [0, 100, B - 1]
    yr = restate.resample(x[idx].cpu(), 44100, 16000)
    assert rel_err(y[idx], yr) < REL
    Xr = restate.stft(yr, 2048, 512)
    assert rel_err(s.stft_data[idx], Xr) < REL
    assert rel_err(mel[idx], restate.mel_spectrogram(Xr, 16000, 80)) < REL
    # resampling is linear and per row: resample(a x) == a resample(x); a second run is bit-equal
    y2 = A.AudioSignal(-0.5 * x, 44100).resample(16000).audio_data
    assert rel_err(y2, -0.5 * y) < 1e-6
    y3 = A.AudioSignal(x, 44100).resample(16000).audio_data
    assert torch.equal(y3, y)
    # the additionally reported (512, 128) parameters
    mel2 = A.AudioSignal(y[idx].clone(), 16000).mel_spectrogram(80, window_length=512, hop_length=128)
    assert rel_err(mel2, restate.mel_spectrogram(restate.stft(yr, 512, 128), 16000, 80)) < REL


@pytest.mark.parametrize("old,new,T", [(441, 160, 50000), (147, 160, 20011), (3, 2, 7000), (3, 1, 9001), (5, 7, 3000),
                                       (1, 2, 4000), (441, 160, 300), (21, 16, 100000)])
def test_resample_mfma_and_valu_kernels_agree(old, new, T):
    """The matrix-core form (at_resample_mfma_f32, odd reduced source rates) and the VALU form
    (at_resample_f32) of the polyphase resampler through the raw C ABI, against the oracle: several
    tiles per row, a partial last frame, rows shorter than one tile, up- and down-sampling."""
    import math
    from audiotools_amd import tables
    lib = _native.lib()
    x = synth.audio_batch(2, 2, T, seed=old + new, gaps=False, sample_rate=old)
    xd = x.cuda().contiguous()
    out_len = int(math.floor(new * T / old))
    st = _native.current_stream(xd.device)
    ref = restate.resample(x, old, new)
    assert ref.shape[-1] == out_len
    assert lib.at_resample_mfma_supported(old, new) == 1
    W, lo, o_, n_, width, NPB, NC = tables.resample_mfma_bank(old, new)
    Wd, lod = torch.from_numpy(W).cuda(), torch.from_numpy(lo).cuda()
    y1 = torch.full((2, 2, out_len), float("nan"), device="cuda")
    rc = lib.at_resample_mfma_f32(_native.ptr(xd), 4, T, _native.ptr(Wd), _native.ptr(lod), old, new, width, NPB, NC,
                                  int(lo.max()), _native.ptr(y1), out_len, st)
    assert rc == 0 and rel_err(y1, ref) < REL
    wg, base, o_, n_, width, NG, LG = tables.resample_grouped_bank(old, new)
    wgd, based = torch.from_numpy(wg).cuda(), torch.from_numpy(base).cuda()
    y2 = torch.full((2, 2, out_len), float("nan"), device="cuda")
    rc = lib.at_resample_f32(_native.ptr(xd), 4, T, _native.ptr(wgd), _native.ptr(based), old, new, width, NG, LG,
                             _native.ptr(y2), out_len, st)
    assert rc == 0 and rel_err(y2, ref) < REL
    assert rel_err(y1, y2.cpu()) < 1e-5
    assert lib.at_resample_mfma_supported(160, 147) == 0      # even reduced source rate: VALU kernel only


@pytest.mark.parametrize("old,new,T,off", [(441, 160, 50000, 0), (441, 160, 50001, 1), (147, 160, 20011, 2), (441, 160, 300, 3),
                                            (441, 160, 16, 0), (147, 80, 30000, 1), (441, 160, 7056 * 3 + 70, 0)])
def test_resample_f16_split_kernel_raw_abi(old, new, T, off):
    """at_resample_f16s_f32 (fp16-split matrix-core form, csrc/resample_f16.hip) through the raw C ABI against the oracle and
    against the float32 matrix-core kernel: several tiles per row and per workgroup, a partial last frame, rows shorter than
    one tile, T = 16, rows whose base address is 4 / 8 / 12 bytes off a 16-byte boundary (the DMA alignment shift), an output
    buffer pre-filled with NaN (every sample written), and a float64 yardstick: no worse than the float32 kernel."""
    import math
    from audiotools_amd import tables
    lib = _native.lib()
    assert lib.at_resample_f16s_supported(old, new) == 1
    x = synth.audio_batch(3, 2, T, seed=old + new + T, gaps=False, sample_rate=old)
    big = torch.zeros(6 * T + 8, device="cuda")
    xd = big[off: off + 6 * T].view(3, 2, T)
    xd.copy_(x)
    assert xd.data_ptr() % 16 == 4 * off
    out_len = int(math.floor(new * T / old))
    st = _native.current_stream(xd.device)
    ref = restate.resample(x, old, new)
    ref64 = restate.resample(x.double(), old, new)
    W, lo, o_, n_, width, NPB, NC, wk = tables.resample_f16_bank(old, new)
    Wd, lod = torch.from_numpy(W.view(np.int32)).cuda(), torch.from_numpy(lo).cuda()
    # (the shipped form is the register-prefetch kernel; the LDS-DMA form it was checked against bit for bit in round 4
    #  lives on in the development build only, tools/rsbench.py)
    y1 = torch.full((3, 2, out_len), float("nan"), device="cuda")
    rc = lib.at_resample_f16s_f32(_native.ptr(xd), 6, T, _native.ptr(Wd), _native.ptr(lod), old, new, width, NPB, NC,
                                  int(lo.max()), wk, _native.ptr(y1), out_len, st)
    assert rc == 0 and torch.isfinite(y1).all() and rel_err(y1, ref) < REL
    W2, lo2, o_, n_, width, NPB2, NC2 = tables.resample_mfma_bank(old, new)
    W2d, lo2d = torch.from_numpy(W2).cuda(), torch.from_numpy(lo2).cuda()
    y2 = torch.full((3, 2, out_len), float("nan"), device="cuda")
    rc = lib.at_resample_mfma_f32(_native.ptr(xd), 6, T, _native.ptr(W2d), _native.ptr(lo2d), old, new, width, NPB2, NC2,
                                  int(lo2.max()), _native.ptr(y2), out_len, st)
    assert rc == 0 and rel_err(y1, y2.cpu()) < 1e-5
    e16 = (y1.cpu().double() - ref64).abs().amax(-1) / ref64.abs().amax(-1)
    e32 = (y2.cpu().double() - ref64).abs().amax(-1) / ref64.abs().amax(-1)
    print(f"resample {old}->{new} T={T}: fp16-split {e16.max():.2e}, f32 MFMA {e32.max():.2e}")
    assert (e16 <= 1.5 * e32 + 3e-7).all()
    # unsupported shapes are refused, not mis-computed
    assert lib.at_resample_f16s_supported(160, 147) == 0 and lib.at_resample_f16s_supported(3, 1) == 0
    assert lib.at_resample_f16s_f32(_native.ptr(xd), 6, T, _native.ptr(Wd), _native.ptr(lod), 160, 147, width, NPB, NC,
                                    int(lo.max()), wk, _native.ptr(y1), out_len, st) == -2


def test_resample_f16_split_nonfinite_and_extreme_rows():
    """Rows the per-tile scale has to cope with: all zeros, 1e-30 and 1e+30 amplitudes, one inf sample (poisons its own
    windows, nothing else of its tile), through AudioSignal.resample (the dispatch picks the fp16-split kernel for 441:160)."""
    T = 60000
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5, 1, T, generator=g)
    x[0] = 0
    x[1] *= 1e-30
    x[2] *= 1e30
    x[3, 0, 20000] = float("inf")
    x[4, 0, :30000] *= 1e-5
    got = A.AudioSignal(x.clone(), 44100).to("cuda").resample(16000).audio_data.cpu()
    ref = restate.resample(x.double(), 44100, 16000)
    assert torch.equal(got[0], torch.zeros_like(got[0]))
    for r in (1, 2, 4):
        assert ((got[r].double() - ref[r]).abs().max() / ref[r].abs().max()) < 1e-6
    quiet = slice(0, 16000 * 29000 // 44100)
    assert ((got[4, 0, quiet].double() - ref[4, 0, quiet]).abs().max() / ref[4, 0, quiet].abs().max()) < 2e-6
    clean = torch.isfinite(ref[3, 0])
    assert torch.isfinite(got[3, 0][clean]).all() and not torch.isfinite(got[3, 0][16000 * 20000 // 44100])
    assert ((got[3, 0][clean].double() - ref[3, 0][clean]).abs().max() / ref[3, 0][clean].abs().max()) < 1e-6


@pytest.mark.parametrize("n_fft,hop,wt", [(4096, 1024, "hann"), (8192, 2048, "sqrt_hann"), (16384, 4096, "hann"), (400, 160, "hann"),
                                          (1200, 300, "sqrt_hann"), (1920, 480, "hann"), (100, 33, "hann"), (4096, 1000, "average"),
                                          (882, 441, "hann"), (1764, 441, "hann")])
def test_stft_generic_sizes_vs_oracle(n_fft, hop, wt):
    """Transform sizes beyond the fused wave-FFT kernels (the default window at 96 / 192 kHz is
    4096 / 8192, audio_signal.py:1066-1070; speech front ends use 400 / 1200 / 1920; 20 / 40 ms at
    44.1 kHz are 882 / 1764 = 2 * 3^2 * 7^2 (* 2)): the mixed-radix
    workgroup FFT of csrc/stft_generic.hip, forward and inverse, against the oracle."""
    assert kernels.stft_native_supported(n_fft) and not kernels.stft_fused_supported(n_fft)
    T = 5 * n_fft + 137
    x = synth.audio_batch(2, 2, T, seed=n_fft, gaps=False)
    s = A.AudioSignal(x.clone(), 16000).to("cuda")
    X = s.stft(n_fft, hop, wt)
    ref = restate.stft(x, n_fft, hop, wt)
    assert X.shape == ref.shape and X.stride()[-2] == 1
    assert rel_err(X, ref) < REL
    if wt != "average" or hop * 4 <= n_fft:
        y = s.istft(n_fft, hop, wt).audio_data
        yr = restate.istft(ref, n_fft, hop, wt, False, T)
        assert rel_err(y, yr) < REL and float((y.cpu() - x).abs().max()) < 1e-4


@pytest.mark.parametrize("sr,n_fft,hop,T", [(16000, 400, 160, 32000 + 3), (16000, 400, 160, 400 + 5 * 160), (16000, 400, 100, 20000),
                                            (24000, 1200, 300, 48000), (48000, 1920, 480, 96000 + 1), (8000, 100, 33, 12345),
                                            (44100, 882, 441, 44100)])
def test_stft_generic_many_frames_per_tile(sr, n_fft, hop, T):
    """The run-time-plan tile holds as many frames as fit 4096 complex points (round 4: 20 at n_fft 400, 6 at 1200, 4 at
    1920, 64 at 100): rows long enough for full tiles, rows whose frame count is not a multiple of the tile (the last tile
    overlaps its predecessor), a row that holds fewer frames than a tile, spectrum and fused mel against the oracle."""
    x = synth.audio_batch(3, 2, T, seed=T + n_fft, gaps=False, sample_rate=sr)
    s = A.AudioSignal(x.clone(), sr).to("cuda")
    ref = restate.stft(x, n_fft, hop, "hann")
    assert rel_err(s.stft(n_fft, hop, "hann"), ref) < REL
    mel = s.mel_spectrogram(40, window_length=n_fft, hop_length=hop, window_type="hann")
    assert rel_err(mel, restate.mel_spectrogram(ref, sr, 40)) < REL
    assert rel_err(s.stft_data, ref) < REL
    # ... and back: the inverse frames share tiles the same way (istft_frames_generic_tiled_kernel; tiles run across rows,
    # the last one is moved back to hold whole frames), against the oracle's istft of the oracle's spectrum and against x
    y = s.istft(n_fft, hop, "hann").audio_data
    assert rel_err(y, restate.istft(ref, n_fft, hop, "hann", False, T)) < REL
    assert float((y.cpu() - x).abs().max()) < 1e-4


@pytest.mark.parametrize("n_fft,T,B", [(4096, 96000 + 1, 3), (4096, 3 * 1024, 2), (4096, 200000, 5), (8192, 9 * 8192 + 5, 2),
                                       (8192, 6000, 1)])
def test_istft_tiled_sizes(n_fft, T, B):
    """The tiled inverse of the 96 / 192 kHz default sizes (csrc/stft_generic.hip, overlap-add in an LDS ring): odd and
    even lengths, rows shorter than a run / than one frame, several runs per row (200 000 samples = 196 frames > 96
    segments), against torch.istft on the same spectrum and against the frame-buffer + gather path."""
    hop = n_fft // 4
    x = synth.audio_batch(B, 2, T, seed=n_fft + T, gaps=False)
    s = A.AudioSignal(x.clone(), 96000).to("cuda")
    X = s.stft(n_fft, hop, "hann").clone()
    win = tables.window("hann", n_fft, "cuda")
    y = kernels.istft(X, win, n_fft, hop, T)
    ref = torch.istft(X.reshape(-1, X.shape[-2], X.shape[-1]).cpu(), n_fft, hop, window=win.cpu(), center=True, length=T)
    assert rel_err(y.reshape(ref.shape), ref) < REL and float((y.cpu() - x).abs().max()) < 1e-4
    # a modified spectrum (no longer the transform of any signal) exercises every frame's own contribution
    g = torch.Generator(device="cuda").manual_seed(1)
    X2 = X * (0.5 + torch.rand(X.shape, device="cuda", generator=g))
    y2 = kernels.istft(X2, win, n_fft, hop, T)
    ref2 = torch.istft(X2.reshape(-1, X.shape[-2], X.shape[-1]).cpu(), n_fft, hop, window=win.cpu(), center=True, length=T)
    assert rel_err(y2.reshape(ref2.shape), ref2) < REL


@pytest.mark.parametrize("n_fft,hop,T,B", [(400, 400, 4000, 2), (400, 200, 400, 3), (400, 200, 1000, 1), (1200, 600, 2400 + 7, 2),
                                          (1920, 96, 12000, 1), (320, 40, 3000, 2), (512, 100, 100000, 2), (400, 160, 160 * 700, 4),
                                          (1000, 250, 30000, 3)])
def test_istft_one_pass_edge_shapes(n_fft, hop, T, B):
    """The one-pass inverse of the run-time sizes (istft_generic_ola_kernel) at its corners: hop = n_fft (no history at
    all), one to three frames per row, a history of nineteen / seven frames (hop = n_fft / 20, n_fft / 8), a power-of-two
    size with a hop the fused kernels do not take, rows long enough for several runs with a warm-up tile each; modified
    spectra against torch.istft with a rectangular window where Hann would violate NOLA."""
    wt = "hann" if n_fft % hop == 0 and n_fft // hop >= 2 else None
    win = tables.window("hann", n_fft, "cuda") if wt else torch.ones(n_fft, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(n_fft + hop)
    n_frames = 1 + T // hop
    X = torch.randn(B, 2, n_fft // 2 + 1, n_frames, dtype=torch.complex64, device="cuda", generator=g)
    X = X.transpose(2, 3).contiguous().transpose(2, 3)            # bin-contiguous, as stft() hands it over
    y = kernels.istft(X, win, n_fft, hop, T)
    ref = torch.istft(X.reshape(-1, X.shape[-2], X.shape[-1]).cpu(), n_fft, hop, window=win.cpu(), center=True, length=T)
    assert y.shape[-1] == T and rel_err(y.reshape(ref.shape), ref) < REL


def test_stft_generic_match_stride_and_mel():
    x = synth.audio_batch(2, 1, 40000 + 13, seed=3, gaps=False)
    s = A.AudioSignal(x.clone(), 96000).to("cuda")
    assert s.stft_params.window_length == 4096                      # the reference's default at 96 kHz
    X = s.stft(match_stride=True, window_type="sqrt_hann")
    ref = restate.stft(x, 4096, 1024, "sqrt_hann", True, "reflect")
    assert rel_err(X, ref) < REL
    y = s.istft(match_stride=True, window_type="sqrt_hann").audio_data
    yr = restate.istft(ref, 4096, 1024, "sqrt_hann", True, x.shape[-1])
    assert y.shape == x.shape == yr.shape and rel_err(y, yr) < REL      # (edges are not x: 2 frames were dropped)
    s2 = A.AudioSignal(x.clone(), 96000).to("cuda")                 # (istft() above replaced s.audio_data)
    mel = s2.mel_spectrogram(80)                                    # dense basis on the native spectrum
    Xr = restate.stft(x, 4096, 1024)
    assert rel_err(mel, restate.mel_spectrogram(Xr, 96000, 80)) < REL
    assert rel_err(s2.stft_data, Xr) < REL


@pytest.mark.parametrize("sr,n_fft,hop,n_mels", [(96000, 4096, 1024, 80), (192000, 8192, 2048, 128), (16000, 400, 160, 40),
                                                 (24000, 1200, 300, 80), (48000, 1920, 480, 64), (44100, 882, 441, 20),
                                                 (96000, 4096, 1000, 7), (96000, 4096, 1024, 256)])
def test_generic_sizes_fused_mel(sr, n_fft, hop, n_mels):
    """mel_spectrogram at the transform sizes of csrc/stft_generic.hip: the banded filterbank is applied inside the
    tiled mixed-radix kernel (audio_signal.py:1355-1368 is abs + a dense matmul over the stored spectrum); odd
    lengths, edge tiles, band counts from 7 (bands hundreds of bins wide: several per-wave pieces per band in the
    hand-addressed tile's lane-level sums) to 256 (854 chunk tasks per tile: more than that tile's three per thread, so the
    launcher falls back to the generic tile)."""
    T = 9 * n_fft + 211
    x = synth.audio_batch(3, 2, T, seed=n_fft + n_mels, gaps=False, sample_rate=sr)
    s = A.AudioSignal(x.clone(), sr).to("cuda")
    mel = s.mel_spectrogram(n_mels, window_length=n_fft, hop_length=hop, window_type="hann")
    Xr = restate.stft(x, n_fft, hop)
    assert mel.shape == (3, 2, n_mels, Xr.shape[-1])
    assert rel_err(s.stft_data, Xr) < REL
    assert rel_err(mel, restate.mel_spectrogram(Xr, sr, n_mels)) < REL
    # the tiled kernel and the one-frame-per-workgroup kernel of round 2 agree on the spectrum
    if n_fft <= 8192:
        assert rel_err(s.stft_data, A.AudioSignal(x.clone(), sr).to("cuda").stft(n_fft, hop, "hann")) < 1e-6


@pytest.mark.parametrize("n_fft,T", [(2048, 40000), (512, 9000 + 7)])
def test_spec_polar_elem_kernel(n_fft, T):
    """Per-element polar edits (csrc/specedit.hip spec_polar_elem_kernel) against the torch
    formulation of dsp.py:354-370 / transforms.py:1478-1494: phase rotation by a full tensor, and
    the noise refill of masked holes."""
    x = synth.audio_batch(3, 2, T, seed=n_fft, gaps=False)
    s = A.AudioSignal(x.clone(), 44100).to("cuda")
    X = s.stft(n_fft, n_fft // 4).clone()
    g = torch.Generator(device="cuda").manual_seed(5)
    sh = torch.randn(X.shape, device="cuda", generator=g)
    ref = X.abs() * torch.exp(1j * (X.angle() + sh))
    assert rel_err(kernels.spec_polar_elem(X, sh), ref) < REL
    assert rel_err(kernels.spec_polar_elem(X, sh[0]), X.abs() * torch.exp(1j * (X.angle() + sh[0]))) < REL   # (C, F, N) broadcast
    # refill: zero a time span and a band, then fill
    Xh = X.clone()
    Xh[..., 10:20] = 0
    Xh[:, :, 30:60, :] = 0
    a = torch.randn(X.shape, device="cuda", generator=g)
    b = torch.randn(X.shape, device="cuda", generator=g)
    got = kernels.spec_polar_elem(Xh, b, a)
    hole = Xh == 0
    want = torch.where(hole, a.abs() * torch.exp(1j * b), Xh)   # magnitude setter then phase setter: |a| e^{ib}
    assert rel_err(got, want) < 1e-6 and torch.equal(got[~hole], Xh[~hole]) and int(hole.sum()) > 0


def test_noise_transforms_fill_holes_on_device():
    from audiotools_amd import transforms as tfm
    x = synth.audio_batch(4, 1, 44100, seed=12, gaps=False)
    for t in (tfm.TimeNoise(), tfm.FrequencyNoise(), tfm.CorruptPhase()):
        sig = A.AudioSignal(x.clone(), 44100)
        kw = t.batch_instantiate([1, 2, 3, 4], sig)
        out = t(sig.clone().to("cuda"), **A.util.prepare_batch(kw, "cuda"))
        assert out.audio_data.shape == x.shape and torch.isfinite(out.audio_data).all()
        assert float((out.audio_data.cpu() - x).abs().max()) > 1e-3          # something changed
    # corrupt_phase() with a scalar scale keeps the magnitudes
    s = A.AudioSignal(x.clone(), 44100).to("cuda")
    m0 = s.magnitude.clone()
    s.corrupt_phase(0.3)
    assert rel_err(s.magnitude, m0) < 1e-5 and float((s.phase - torch.angle(s.stft_data)).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------
# Structured inputs against float64, bounded by torch's own float32 error
# ------------------------------------------------------------------------------------------------
def _bounded_by_torch(got, f32, f64, what, slack=2.0, floor=1e-6):
    """Per row: err(HIP vs float64) <= slack * err(torch float32 vs float64) + floor, and < REL.
    floor = 1e-6 (8 float32 ulps of the row maximum): on rows where torch's float32 result happens to be almost
    exact (an impulse train through its FFT convolution: 8e-8) a pure multiple of its error would demand less
    than the rounding noise of ANY float32 block-FFT evaluation (measured here: 6e-7, profiles/r03_structured_parity.txt)."""
    e_hip = row_errs(got.double(), f64)
    e_t32 = row_errs(f32.double(), f64)
    print(f"{what}: per-row error vs float64  HIP {['%.1e' % v for v in e_hip.tolist()]}  torch f32 {['%.1e' % v for v in e_t32.tolist()]}")
    assert bool((e_hip < REL).all()), (what, e_hip)
    assert bool((e_hip <= slack * e_t32 + floor).all()), (what, e_hip, e_t32)


@pytest.mark.parametrize("sr,n_fft,hop", [(44100, 2048, 512), (16000, 512, 128), (48000, 1024, 256)])
def test_stft_mel_structured_inputs(sr, n_fft, hop):
    """stft + mel_spectrogram on tonal (100 dB between partials) / pink / swept / burst / impulse / DC+Nyquist rows."""
    from audiotools_amd import tables
    x = synth.structured_batch(40000, sr)
    win64 = torch.from_numpy(tables.window_np("hann", n_fft)).double()
    X64 = torch.stft(x.double().reshape(-1, x.shape[-1]), n_fft, hop, window=win64, center=True, pad_mode="reflect",
                     return_complex=True).reshape(x.shape[0], 1, n_fft // 2 + 1, -1)
    X32 = torch.stft(x.reshape(-1, x.shape[-1]), n_fft, hop, window=win64.float(), center=True, pad_mode="reflect",
                     return_complex=True).reshape(X64.shape)
    s = A.AudioSignal(x.clone(), sr).to("cuda")
    X = s.stft(n_fft, hop, "hann")
    _bounded_by_torch(torch.view_as_real(X.cpu()), torch.view_as_real(X32), torch.view_as_real(X64), f"stft {n_fft}/{hop}")
    # per FRAME as well: the burst row has 100 dB between its frames, the row maximum hides the quiet ones
    Xn = torch.view_as_real(X.cpu()).double().permute(0, 1, 3, 2, 4)       # (B, C, N, F, 2): rows = frames
    e_fr = row_errs(Xn, torch.view_as_real(X64).permute(0, 1, 3, 2, 4), lead=3)
    e_fr_t = row_errs(torch.view_as_real(X32).double().permute(0, 1, 3, 2, 4), torch.view_as_real(X64).permute(0, 1, 3, 2, 4), lead=3)
    assert float(e_fr.max()) < REL and bool((e_fr <= 2.0 * e_fr_t.max() + 3e-7).all()), (float(e_fr.max()), float(e_fr_t.max()))
    basis = torch.from_numpy(tables.mel_filters_np(sr, n_fft, 80, 0.0, None))
    mel64 = (X64.abs().transpose(2, 3) @ basis.double().T).transpose(2, 3)
    mel32 = (X32.abs().transpose(2, 3) @ basis.T).transpose(2, 3)
    mel = A.AudioSignal(x.clone(), sr).to("cuda").mel_spectrogram(80, window_length=n_fft, hop_length=hop, window_type="hann")
    _bounded_by_torch(mel.cpu(), mel32, mel64, f"mel {n_fft}/{hop}")


@pytest.mark.parametrize("sr,n_fft,hop", [(44100, 2048, 512), (16000, 512, 128), (22050, 1024, 256), (16000, 400, 160),
                                          (48000, 1920, 480)])
def test_istft_structured_inputs(sr, n_fft, hop):
    from audiotools_amd import tables
    x = synth.structured_batch(40000, sr)
    T = x.shape[-1]
    win = torch.from_numpy(tables.window_np("hann", n_fft))
    Xc = torch.stft(x.reshape(-1, T), n_fft, hop, window=win, center=True, pad_mode="reflect", return_complex=True)
    y64 = torch.istft(Xc.to(torch.complex128), n_fft, hop, window=win.double(), center=True, length=T).reshape(x.shape)
    y32 = torch.istft(Xc, n_fft, hop, window=win, center=True, length=T).reshape(x.shape)
    s = A.AudioSignal(x.clone(), sr).to("cuda")
    s.stft_data = Xc.reshape(x.shape[0], 1, n_fft // 2 + 1, -1).to("cuda")
    got = s.istft(n_fft, hop, "hann").audio_data
    _bounded_by_torch(got.cpu(), y32, y64, f"istft {n_fft}/{hop}")


@pytest.mark.parametrize("old,new", [(44100, 16000), (16000, 22050), (48000, 44100)])
def test_resample_structured_inputs(old, new):
    """Polyphase resampler (VALU and matrix-core forms) with the reference's float32 taps applied in float64."""
    from oracle.leaves import julius_leaf
    x = synth.structured_batch(30011, old)
    m = julius_leaf.ResampleFrac(old, new)
    xp = torch.nn.functional.pad(x.double().reshape(-1, 1, x.shape[-1]), (m._width, m._width + m.old_sr), mode="replicate")
    ys = torch.nn.functional.conv1d(xp, m.kernel.double(), stride=m.old_sr)
    n_out = int(np.floor(m.new_sr * x.shape[-1] / m.old_sr))
    y64 = ys.transpose(1, 2).reshape(x.shape[0], 1, -1)[..., :n_out]
    y32 = restate.resample(x, old, new)
    got = A.AudioSignal(x.clone(), old).to("cuda").resample(new).audio_data
    _bounded_by_torch(got.cpu(), y32, y64, f"resample {old}->{new}")


@pytest.mark.parametrize("highpass", [False, True])
def test_sinc_filters_structured_inputs(highpass):
    """low_pass / high_pass (direct and overlap-save forms) on structured rows, per-item cutoffs."""
    from oracle.leaves import julius_leaf
    sr = 44100
    x = synth.structured_batch(30001, sr)
    cut = torch.tensor([4000.0, 16000.0, 300.0, 8000.0, 1000.0, 100.0])
    s = A.AudioSignal(x.clone(), sr).to("cuda")
    got = (s.high_pass(cut) if highpass else s.low_pass(cut)).audio_data
    y32 = restate.high_pass(x, cut, sr) if highpass else restate.low_pass(x, cut, sr)
    y64 = torch.empty(x.shape, dtype=torch.float64)
    for i in range(x.shape[0]):
        f = julius_leaf.LowPassFilters([float((cut[i] / sr).float())], zeros=51)
        xp = torch.nn.functional.pad(x[i].double()[:, None], (f.half_size, f.half_size), mode="replicate")
        lp = torch.nn.functional.conv1d(xp, f.filters.double())[:, 0]
        y64[i] = (x[i].double() - lp) if highpass else lp
    _bounded_by_torch(got.cpu(), y32, y64, "high_pass" if highpass else "low_pass")


# ------------------------------------------------------------------------------------------------
# STFT-domain edits folded into the inverse transform (csrc/istft.hip EDIT)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,T", [(44100, 60000 + 7), (16000, 20000)])
@pytest.mark.parametrize("match_stride", [False, True])
def test_deferred_spectral_edits_equal_eager(sr, T, match_stride):
    """Inside a SpectralTransform a per-item mask / phase shift is recorded and applied by the inverse kernel as it
    loads the spectrum (at_istft_edit_f32).  Same audio as the eager edit kernel + plain inverse, stft_data (read
    afterwards) is the eagerly edited spectrum with untouched bins bit-identical, and a new tensor."""
    from audiotools_amd import transforms as tfm
    x = synth.audio_batch(3, 2, T, seed=T, gaps=False, sample_rate=sr)
    kw = dict(match_stride=match_stride, window_type="sqrt_hann") if match_stride else {}
    edits = {
        "mask_frequencies": lambda s: s.mask_frequencies(torch.tensor([300.0, 1000.0, 50.0]), torch.tensor([900.0, 4000.0, 7000.0])),
        "mask_frequencies_val": lambda s: s.mask_frequencies(500.0, 2500.0, val=0.3),
        "mask_timesteps": lambda s: s.mask_timesteps(torch.tensor([0.1, 0.2, 0.0]), torch.tensor([0.3, 0.25, 0.9])),
        "mask_low_magnitudes": lambda s: s.mask_low_magnitudes(torch.tensor([-30.0, -20.0, -45.0])),
        "shift_phase": lambda s: s.shift_phase(torch.tensor([0.5, -2.0, 3.0])),
    }
    for name, edit in edits.items():
        a = A.AudioSignal(x.clone(), sr).to("cuda")
        b = A.AudioSignal(x.clone(), sr).to("cuda")
        Xa = a.stft(**kw).clone()
        b.stft(**kw)
        held = a._stft_data
        tfm._deferring(a, lambda: edit(a))
        assert a._pending_edit is not None, name                 # recorded, not applied
        assert a._stft_data is held and torch.equal(a._stft_data, Xa)
        edit(b)                                                  # eager
        assert b._pending_edit is None
        ya = a.istft(**{k: v for k, v in kw.items()}).audio_data
        yb = b.istft(**{k: v for k, v in kw.items()}).audio_data
        assert a._pending_edit is not None                       # still lazy after the fused inverse
        assert rel_err(ya, yb) < 2e-6, name
        Xe = a.stft_data                                         # reading materialises
        assert a._pending_edit is None and Xe is not held
        assert torch.equal(Xe, b.stft_data), name
        assert torch.equal(held, Xa)                             # the tensor a caller may still hold did not change
    # two edits in a row compose in order (the first is materialised when the second arrives)
    a = A.AudioSignal(x.clone(), sr).to("cuda")
    b = A.AudioSignal(x.clone(), sr).to("cuda")
    a.stft(); b.stft()
    tfm._deferring(a, lambda: a.shift_phase(0.7).mask_frequencies(200.0, 3000.0))
    b.shift_phase(0.7).mask_frequencies(200.0, 3000.0)
    assert rel_err(a.istft().audio_data, b.istft().audio_data) < 2e-6


def test_spectral_transforms_use_the_fused_inverse():
    """FrequencyMask / TimeMask / ShiftPhase / MaskLowMagnitudes through BaseTransform on the HIP path: the edit is
    pending when istft() runs (one pass saved), the result equals the CPU path with the same parameters."""
    from audiotools_amd import transforms as tfm
    sr = 44100
    x = synth.audio_batch(4, 1, 44100, seed=77, gaps=False)
    for t in (tfm.FrequencyMask(), tfm.TimeMask(), tfm.ShiftPhase(), tfm.MaskLowMagnitudes(), tfm.InvertPhase()):
        sig = A.AudioSignal(x.clone(), sr)
        kw = t.batch_instantiate([5, 6, 7, 8], sig)
        ref = t(sig.clone(), **kw).audio_data
        dev = sig.clone().to("cuda")
        calls = []
        orig = kernels.istft
        kernels.istft = lambda *a, **k: (calls.append(k.get("edit") is not None), orig(*a, **k))[1]
        try:
            got = t(dev, **A.util.prepare_batch(kw, "cuda")).audio_data
        finally:
            kernels.istft = orig
        assert calls == [True], (type(t).__name__, calls)
        assert rel_err(got, ref) < REL, type(t).__name__


@pytest.mark.parametrize("nz_batch,amount", [(1, 1.0), (3, torch.tensor([0.5, 1.0, 0.8])), (1, 0.0)])
def test_spectral_gate_kernel_vs_torch_formulation(nz_batch, amount):
    """csrc/specedit.hip spec_gate_kernel (gate bits in LDS, separable tent smoothing, complex product: one pass)
    against the reference's whole-tensor formulation (ml/layers/spectral_gate.py:96-121) evaluated with torch ops ON
    THE SAME DEVICE SPECTRUM, so the only differences are bins whose dB value sits on the threshold."""
    from audiotools_amd.ml.layers import SpectralGate
    sr = 44100
    x = synth.audio_batch(3, 2, 30000 + 11, seed=5, gaps=False)
    nz = 0.02 * torch.randn(nz_batch, 2, 15000, generator=torch.Generator().manual_seed(8))
    gate = SpectralGate(3, 5).to("cuda")
    sig = A.AudioSignal(x.clone(), sr).to("cuda")
    noise = A.AudioSignal(nz.clone(), sr).to("cuda")
    got = gate(sig, noise, amount, n_std=2.0)
    # the torch formulation on the device (the module's own fallback branch)
    saved = kernels.spec_native
    kernels.spec_native = lambda X: False
    try:
        ref = gate(sig, noise, amount, n_std=2.0)
    finally:
        kernels.spec_native = saved
    d = (got.audio_data - ref.audio_data).abs()
    scale = ref.audio_data.abs().amax(-1, keepdim=True)
    assert float((d > 1e-3 * scale).float().mean()) < 1e-3          # isolated threshold flips only
    assert float(d.max() / scale.max()) < 0.05
    if isinstance(amount, float) and amount == 0.0:
        assert rel_err(got.audio_data, ref.audio_data) < 1e-5
    # the gate kernel itself against the formula on a small spectrum, exactly (thresholds far from the data)
    X = torch.view_as_complex(torch.randn(2, 1, 37, 65, 2, generator=torch.Generator().manual_seed(1))).cuda()   # (B, C, N, F) physical
    Xl = X.transpose(2, 3)
    thr = torch.full((1, 1, 65), -3.0)
    tf, tt = gate.tent_f.cpu(), gate.tent_t.cpu()
    Y = kernels.spec_gate(Xl, thr, torch.tensor([1.0, 0.5]), tf, tt)
    db = 20 * Xl.abs().clamp(1e-4).log10()
    g = (db < -3.0).float()
    sm = torch.nn.functional.conv2d(g.reshape(2, 1, 65, 37), torch.outer(tf, tt)[None, None].cuda(), padding=(3, 5)).reshape(2, 1, 65, 37)
    want = Xl * (1 - sm * torch.tensor([1.0, 0.5]).cuda()[:, None, None, None])
    assert rel_err(torch.view_as_real(Y), torch.view_as_real(want)) < 1e-5


def test_lufs_does_not_depend_on_workspace_contents():
    """at_lufs_f32 no longer zero-fills its hop-energy table (every hop that holds samples is written by exactly one
    wave; only signals shorter than a gating block keep the memset): the result must be bit-stable when the recycled
    workspace is full of NaNs -- whole rows, a tail that is not a multiple of the hop, exactly one block, less than one."""
    for T in (441000, 44100 * 3 + 28, 17640, 8000, 4410 * 5, 100000):
        x = synth.audio_batch(6, 2, T, seed=T, gaps=False).cuda() * 0.3
        ref = kernels.integrated_loudness(x, 44100).clone()
        for _ in range(3):
            junk = torch.full((32 * 1024 * 1024,), float("nan"), device="cuda")
            del junk
            assert torch.equal(kernels.integrated_loudness(x, 44100), ref), T
        want = restate.integrated_loudness(x.cpu(), 44100)          # the meter itself (no padding to 0.5 s, no -70 clamp)
        assert float((ref.cpu() - want).abs().max()) < 0.1


def test_tap_design_kernels_match_torch_formulation():
    """at_sinc_taps_f32 / at_eq_taps_f32 (one launch per call) against the whole-table torch formulations they replace
    (kernels.sinc_taps_batched, fx.equalizer_taps): per-item lengths, a zero cutoff (all-zero filter), the zero padding
    of the table, gains over several decades."""
    from audiotools_amd import fx
    cut = torch.tensor([4000.0, 8000.0, 16000.0, 0.0, 24000.0, 123.4, 1000.0]) / 48000
    ref = kernels.sinc_taps_batched(cut.cuda(), 51, host_cutoffs=cut)
    tp, L = kernels.sinc_taps_native(cut.cuda(), 51, host_cutoffs=cut)
    assert L == ref.shape[1] and tp.shape == (7, (L + 7) // 8 * 8)
    assert float((tp[:, :L] - ref).abs().max()) < 2e-7 and not tp[:, L:].any() and not tp[3].any()
    assert float((tp[:, :L].sum(-1)[[0, 1, 2, 4, 5, 6]] - 1).abs().max()) < 1e-5          # unit DC gain
    tp2, L2 = kernels.sinc_taps_native(cut.cuda(), 51)                                       # without the host twin: one sync
    assert L2 == L and torch.equal(tp2, tp)
    with pytest.raises(ValueError):
        kernels.sinc_taps_native(torch.tensor([0.6]).cuda(), 51)
    for sr, nb in ((48000, 6), (44100, 10), (16000, 3)):
        g = torch.Generator().manual_seed(nb)
        w = (10 ** (torch.rand(5, nb, generator=g) * 2 - 1.5)).cuda()
        ref_t, half = fx.equalizer_taps(sr, w)
        bank, half2 = tables.band_split_bank(sr, nb)
        tq, Lq = kernels.eq_taps_native(w, bank.cuda(), half2)
        assert half == half2 and Lq == ref_t.shape[1]
        assert rel_err(tq[:, :Lq], ref_t) < 1e-6 and not tq[:, Lq:].any()


@pytest.mark.parametrize("T", [96000, 40000, 8192, 2048, 512, 8])
def test_alter_drr_register_resident_kernel(T):
    """Round 5: mono impulse responses of up to 98 304 aligned samples are read ONCE (alter_drr_regs_kernel: the row in the
    registers of one workgroup; csrc/irtools.hip) instead of three times.  Against the torch formulation on the CPU (pinned
    to the unmodified reference in tests/test_transforms.py): peaks at the first / last sample, on wave and iteration
    boundaries of the kernel's element assignment, an all-negative row, a tie, a NaN row; the reported peak equals absmax's;
    in place."""
    from audiotools_amd import kernels
    sr = 48000
    g = torch.Generator().manual_seed(T)
    B = 9
    ir = torch.randn(B, 1, T, generator=g) * torch.exp(-torch.arange(T) / (0.2 * T + 1))
    for b, pos in enumerate((0, T - 1, min(255, T - 1), min(256, T - 1), min(2047, T - 1), min(2048, T - 1), T // 2)):
        ir[b, 0, pos] = ir[b].abs().max() * 1.5
    ir[7] = -ir[7].abs() - 0.01                         # every sample negative: the signed arg-max is the least negative one
    if T >= 512:
        ir[8, 0, 100] = 3.0
        ir[8, 0, 300] = 3.0                              # tie: the first index wins
    drr = torch.tensor([0.0, 3.0, 6.0, 10.0, 15.0, 20.0, 25.0, 30.0, 12.0])
    ref = A.AudioSignal(ir.clone(), sr).alter_drr(drr).audio_data
    sig = A.AudioSignal(ir.clone(), sr).to("cuda")
    got = sig.alter_drr(drr.cuda()).audio_data.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    assert rel_err(torch.nan_to_num(got), torch.nan_to_num(ref)) < 1e-5
    t0 = int(sr * 0.0025)
    x = ir.cuda()
    out, vmax, imax = kernels.alter_drr(x, t0, drr.cuda(), want_peak=True)
    pv, pi = kernels.absmax(out, want_index=True)
    same = lambda a, b: bool(((a == b) | (a.isnan() & b.isnan())).all())
    assert same(vmax, pv) and torch.equal(imax, pi)
    assert same(out.cpu(), got)
    if T >= 4:
        xn = x.clone()
        xn[3, 0, T // 3] = float("nan")                  # a NaN sample: torch's max propagates it, the row becomes NaN
        refn = A.AudioSignal(xn.cpu(), sr).alter_drr(drr).audio_data
        gotn = kernels.alter_drr(xn, t0, drr.cuda()).cpu()
        assert torch.equal(torch.isnan(gotn), torch.isnan(refn))


def test_alter_drr_reports_the_peak_absmax_would():
    """at_alter_drr_peak_f32: the output pass of alter_drr also yields max |out| and its first position per row -- what
    apply_ir's convolution asks at_absmax_f32 for next -- for mono and multi-channel impulse responses, a row whose DRR
    solve fails (NaN propagates like torch), and the cache on the signal object is dropped when the samples change."""
    sr = 48000
    g = torch.Generator().manual_seed(3)
    for B, C, T in ((7, 1, 96000), (3, 2, 24000), (2, 1, 9999)):
        ir = (torch.randn(B, C, T, generator=g) * torch.exp(-torch.arange(T) / (0.05 * sr))).cuda()
        drr = (torch.rand(B, generator=g) * 30).cuda()
        same = lambda a, b: bool(((a == b) | (a.isnan() & b.isnan())).all())     # (a failed DRR solve is a NaN row)
        out, vmax, imax = kernels.alter_drr(ir, int(sr * 0.0025), drr, want_peak=True)
        assert same(out, kernels.alter_drr(ir, int(sr * 0.0025), drr))
        pv, pi = kernels.absmax(out, want_index=True)
        assert same(vmax, pv) and torch.equal(imax, pi)
    s = A.AudioSignal(ir.clone(), sr)
    s.alter_drr(drr)
    assert s._peak_of is not None and s._peak_of[0] is s.audio_data
    s.audio_data = s.audio_data * 2
    assert s._peak_of is None
