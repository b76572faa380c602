#!/usr/bin/env python
"""Forward + backward of a magnitude loss through stft(): native kernels vs torch.stft autograd on the GPU.

usage: gradbench.py [B [case]]    case: all (default) | stft | mel | dacmel | msstft | sisdr (its own shapes, whatever B) | mse | widemel"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import audiotools_amd as A
from audiotools_amd import spectral
B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
CASE = sys.argv[2] if len(sys.argv) > 2 else "all"
x = (0.1 * torch.randn(B, 2, 441000, device="cuda")).clamp_(-1, 1)

def run(native):
    saved = spectral._native_autograd_ok
    if not native:
        spectral._native_autograd_ok = lambda *a: False
    try:
        def fn():
            xa = x.clone().requires_grad_(True)
            X = A.AudioSignal(xa, 44100).stft()
            X.abs().sum().backward()
            return xa.grad
        fn(); torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(3): g = fn()
        torch.cuda.synchronize()
        print(f"stft fwd + |X|.sum() bwd, B={B} ({'native' if native else 'torch.stft'}): {(time.perf_counter() - t0) / 3 * 1e3:8.2f} ms", flush=True)
        return g
    finally:
        spectral._native_autograd_ok = saved

if CASE in ("all", "stft"):
    g1 = run(True); g2 = run(False)
    print("grad rel diff", float((g1 - g2).abs().max() / g2.abs().max()))


def run_mel(native):
    saved = spectral._native_autograd_ok
    if not native:
        spectral._native_autograd_ok = lambda *a: False
    try:
        def fn():
            xa = x.clone().requires_grad_(True)
            mel = A.AudioSignal(xa, 44100).mel_spectrogram(80)
            mel.clamp(1e-5).log10().sum().backward()
            return xa.grad
        fn(); torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(3): g = fn()
        torch.cuda.synchronize()
        print(f"log-mel loss fwd + bwd, B={B} ({'native' if native else 'torch.stft'}): {(time.perf_counter() - t0) / 3 * 1e3:8.2f} ms", flush=True)
        return g
    finally:
        spectral._native_autograd_ok = saved

if CASE in ("all", "mel"):
    m1 = run_mel(True); m2 = run_mel(False)
    print("mel grad rel diff", float((m1 - m2).abs().max() / m2.abs().max()))


def run_dac_mel(native):
    """The 7-scale MelSpectrogramLoss of the Descript Audio Codec recipe, estimate vs reference."""
    from audiotools_amd import metrics
    loss = metrics.spectral.MelSpectrogramLoss(n_mels=[5, 10, 20, 40, 80, 160, 320], window_lengths=[32, 64, 128, 256, 512, 1024, 2048],
                                               mel_fmin=[0] * 7, mel_fmax=[None] * 7, pow=1.0, mag_weight=0.0)
    xs, ys = x[:32], x[32:64].clone()
    saved = spectral._native_autograd_ok
    if not native:
        spectral._native_autograd_ok = lambda *a: False
    try:
        def fn():
            xa = xs.clone().requires_grad_(True)
            loss(A.AudioSignal(xa, 44100), A.AudioSignal(ys, 44100)).backward()
            return xa.grad
        fn(); torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(3): g = fn()
        torch.cuda.synchronize()
        print(f"7-scale MelSpectrogramLoss fwd + bwd, B=32x2chx10s ({'native' if native else 'torch.stft'}): {(time.perf_counter() - t0) / 3 * 1e3:8.2f} ms", flush=True)
        return g
    finally:
        spectral._native_autograd_ok = saved

if CASE in ("all", "dacmel"):
    d1 = run_dac_mel(True); d2 = run_dac_mel(False)
    print("7-scale grad rel diff", float((d1 - d2).abs().max() / d2.abs().max()))


MODES = (False, True, "waveform")    # unfused, fused with G + native adjoint, fused with the waveform gradient in-kernel


def run_dac_mel_fused(rounds=5, reps=10):
    """The same 7-scale loss, forward + backward: fused=True (csrc/meldist.hip) and fused="waveform" against fused=False, alternating in one
    process, every window timed with HIP events; then the kernel alone per scale: with G, without, with dx (waveform mode)."""
    from audiotools_amd import kernels, metrics, tables
    mels, wins = [5, 10, 20, 40, 80, 160, 320], [32, 64, 128, 256, 512, 1024, 2048]
    xs, ys = x[:32], (x[32:64] if B >= 64 else x[:32].flip(0)).clone()
    losses = {f: metrics.spectral.MelSpectrogramLoss(n_mels=mels, window_lengths=wins, mel_fmin=[0] * 7, mel_fmax=[None] * 7,
                                                     pow=1.0, mag_weight=0.0, fused=f) for f in MODES}

    def fn(fused):
        xa = xs.clone().requires_grad_(True)
        losses[fused](A.AudioSignal(xa, 44100), A.AudioSignal(ys, 44100)).backward()
        return xa.grad

    grads = {f: fn(f) for f in MODES}          # warm-up of both paths (code objects, allocator, tables)
    times = {f: [] for f in MODES}
    for _ in range(rounds):
        for f in MODES:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                fn(f)
            t1.record()
            t1.synchronize()
            times[f].append(t0.elapsed_time(t1) / reps)
    for f in MODES:
        ts = sorted(times[f])
        print(f"7-scale MelSpectrogramLoss fwd + bwd, 32x2chx10s, fused={f}: median {ts[len(ts) // 2]:8.2f} ms  "
              f"(min {ts[0]:.2f}, max {ts[-1]:.2f}; {rounds} windows of {reps})", flush=True)
    for f in MODES[1:]:
        print(f"fused={f} vs unfused grad rel diff", float((grads[f] - grads[False]).abs().max() / grads[False].abs().max()))
    S = xs.numel() * 4
    for n_mels, n_fft in zip(mels, wins):
        win = A.AudioSignal.get_window("hann", n_fft, str(xs.device))
        tb = tables.mel_dist_tables(44100, n_fft, n_mels, 0, None, xs.device)
        for want in (True, False, "dx", "G+adjoint"):
            call = lambda: kernels.mel_distance(xs, ys, win, n_fft, n_fft // 4, tb, n_mels, 1e-5, 1.0, 1e-9, 0.0, want)
            if want == "dx":
                call = lambda: kernels.mel_distance_dx(xs, ys, win, n_fft, n_fft // 4, tb, n_mels, 1e-5, 1.0, 1e-9, 0.0)
            if want == "G+adjoint":     # what the waveform mode replaces: the G kernel, at_stft_adjoint_f32, the clone and the folds
                call = lambda: kernels.stft_adjoint(kernels.mel_distance(xs, ys, win, n_fft, n_fft // 4, tb, n_mels, 1e-5, 1.0, 1e-9, 0.0, True)[1],
                                                    win, n_fft, n_fft // 4, xs.shape[-1])
            call()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(50):
                call()
            t1.record()
            t1.synchronize()
            ms = t0.elapsed_time(t1) / 50
            nbytes = 2 * S + {True: 4 * S, False: 0, "dx": S}.get(want, 12 * S)     # G+adjoint: 4 S out, 4 S in, ~4 S of OLA, clone, folds
            print(f"at_mel_dist_f32 n_fft={n_fft} n_mels={n_mels} out={ {True: 'G', False: 'none'}.get(want, want) }: {ms:7.3f} ms, {nbytes / ms / 1e6:.0f} GB/s of its {nbytes / 1e9:.2f} GB", flush=True)


if CASE in ("all", "dacmel"):
    run_dac_mel_fused()


def run_msstft(rounds=5, reps=20):
    """MultiScaleSTFTLoss at its default scales (2048, 512), estimate vs target of 32 x 2 ch x 10 s each, forward + backward:
    fused=True (csrc/stftdist.hip) and fused="waveform" (csrc/dist_ola.h) against fused=False, alternating in one process, every
    window timed with HIP events."""
    from audiotools_amd import metrics
    xs, ys = x[:32], (x[32:64] if B >= 64 else x[:32].flip(0)).clone()
    losses = {f: metrics.spectral.MultiScaleSTFTLoss(fused=f) for f in MODES}

    def fn(fused):
        xa = xs.clone().requires_grad_(True)
        losses[fused](A.AudioSignal(xa, 44100), A.AudioSignal(ys, 44100)).backward()
        return xa.grad

    grads = {f: fn(f) for f in MODES}          # warm-up of both paths (code objects, allocator, tables)
    times = {f: [] for f in MODES}
    for _ in range(rounds):
        for f in MODES:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                fn(f)
            t1.record()
            t1.synchronize()
            times[f].append(t0.elapsed_time(t1) / reps)
    for f in MODES:
        ts = sorted(times[f])
        print(f"MultiScaleSTFTLoss [2048, 512] fwd + bwd, 32x2chx10s, fused={f}: median {ts[len(ts) // 2]:8.2f} ms  "
              f"(min {ts[0]:.2f}, max {ts[-1]:.2f}; {rounds} windows of {reps})", flush=True)
    # what the fused path has to move: per scale 2 S in, G out and in (4 S each way, complex64 at hop n/4), ~1 S out
    S = xs.numel() * 4
    med = sorted(times[True])[rounds // 2]
    print(f"fused path: {2 * 11 * S / 1e9:.2f} GB by its byte budget (11 S per scale) -> {2 * 11 * S / med / 1e6:.0f} GB/s end to end")
    for f in MODES[1:]:
        print(f"fused={f} vs unfused grad rel diff", float((grads[f] - grads[False]).abs().max() / grads[False].abs().max()))

    # the kernel alone (both scales, with and without G)
    from audiotools_amd import kernels
    for n_fft in (2048, 512):
        win = A.AudioSignal.get_window("hann", n_fft, str(xs.device))
        for want in (True, False, "dx", "G+adjoint"):
            call = lambda: kernels.stft_distance(xs, ys, win, n_fft, n_fft // 4, 1e-5, 2.0, 1e-9, 1e-9, want)
            if want == "dx":
                call = lambda: kernels.stft_distance_dx(xs, ys, win, n_fft, n_fft // 4, 1e-5, 2.0, 1e-9, 1e-9)
            if want == "G+adjoint":     # what the waveform mode replaces: the G kernel, at_stft_adjoint_f32, the clone and the folds
                call = lambda: kernels.stft_adjoint(kernels.stft_distance(xs, ys, win, n_fft, n_fft // 4, 1e-5, 2.0, 1e-9, 1e-9, True)[1],
                                                    win, n_fft, n_fft // 4, xs.shape[-1])
            call()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(50):
                call()
            t1.record()
            t1.synchronize()
            ms = t0.elapsed_time(t1) / 50
            nbytes = 2 * S + {True: 4 * S, False: 0, "dx": S}.get(want, 12 * S)     # G+adjoint: 4 S out, 4 S in, ~4 S of OLA, clone, folds
            print(f"at_stft_dist_f32 n_fft={n_fft} out={ {True: 'G', False: 'none'}.get(want, want) }: {ms:7.3f} ms, {nbytes / ms / 1e6:.0f} GB/s of its {nbytes / 1e9:.2f} GB", flush=True)


if CASE in ("all", "msstft"):
    run_msstft()


def _timed(call, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        call()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def run_sisdr(shape, rounds=7, reps=20):
    """SISDRLoss forward + backward (gradient of the estimate), fused=True (csrc/wavedist.hip) against fused=False, alternating in
    one process, every window timed with HIP events; then the two streaming kernels alone next to torch's copy_ of one signal."""
    from audiotools_amd import kernels, metrics
    g = torch.Generator(device="cuda").manual_seed(3)
    ref = (0.1 * torch.randn(shape, device="cuda", generator=g)).clamp_(-1, 1)
    est = 0.7 * ref + 0.01 * torch.randn(shape, device="cuda", generator=g)
    losses = {f: metrics.distance.SISDRLoss(fused=f) for f in (False, True)}

    def fn(fused):
        ea = est.detach().requires_grad_(True)
        loss = losses[fused](ref, ea)
        loss.backward()
        return loss.detach(), ea.grad

    out = {f: fn(f) for f in (False, True)}         # warm-up of both paths
    times = {f: [] for f in (False, True)}
    for _ in range(rounds):
        for f in (False, True):
            times[f].append(_timed(lambda: fn(f), reps))
    for f in (False, True):
        ts = sorted(times[f])
        print(f"SISDRLoss fwd + bwd {tuple(shape)}, fused={f}: median {ts[len(ts) // 2]:8.3f} ms  (min {ts[0]:.3f}, max {ts[-1]:.3f}; "
              f"{rounds} windows of {reps})", flush=True)
    print(f"loss fused {float(out[True][0]):.6f} unfused {float(out[False][0]):.6f}; grad rel diff "
          f"{float((out[True][1] - out[False][1]).abs().max() / out[False][1].abs().max()):.2e}")
    S = ref.numel() * 4
    _, coef, _ = kernels.sisdr(ref, est)
    go = torch.full((shape[0], 1), 1.0 / shape[0], device="cuda")
    dst = torch.empty_like(ref)
    for name, call, nbytes in (("sisdr sums + finish", lambda: kernels.sisdr(ref, est), 2 * S),
                               ("sisdr grad (est)", lambda: kernels.sisdr_grad(ref, est, coef, go, False, True), 3 * S),
                               ("sisdr grad (both)", lambda: kernels.sisdr_grad(ref, est, coef, go, True, True), 4 * S),
                               ("torch copy_", lambda: dst.copy_(ref), 2 * S)):
        call()
        ts = sorted(_timed(call, 50) for _ in range(5))
        print(f"{name} {tuple(shape)}: median {ts[2]:7.4f} ms, {nbytes / ts[2] / 1e6:.0f} GB/s of its {nbytes / 1e9:.4f} GB", flush=True)


if CASE in ("all", "sisdr"):
    for shape in ((64, 1, 441000), (8, 1, 16000)):
        run_sisdr(shape)


def run_mse(rounds=5):
    """The squared-error recipes, forward + backward w.r.t. the estimate: MultiScaleSTFTLoss(loss_fn=nn.MSELoss()) at the default
    scales and the 7-scale DAC mel recipe with nn.MSELoss(), fused=False / True / "waveform" alternating in one process, every window
    between two HIP events; first the whole step, then every scale alone (a one-scale loss: what _fused_scale decides per scale)."""
    from torch import nn
    from audiotools_amd import metrics
    mels, wins = [5, 10, 20, 40, 80, 160, 320], [32, 64, 128, 256, 512, 1024, 2048]
    xs, ys = x[:32], (x[32:64] if B >= 64 else x[:32].flip(0)).clone()

    def stft_loss(f, w=(2048, 512)):
        return metrics.spectral.MultiScaleSTFTLoss(window_lengths=list(w), loss_fn=nn.MSELoss(), fused=f)

    def mel_loss(f, m=mels, w=wins):
        return metrics.spectral.MelSpectrogramLoss(n_mels=list(m), window_lengths=list(w), mel_fmin=[0] * len(w), mel_fmax=[None] * len(w),
                                                   pow=1.0, mag_weight=0.0, loss_fn=nn.MSELoss(), fused=f)

    cases = [("MSE MultiScaleSTFTLoss [2048, 512]", stft_loss, 20), ("MSE 7-scale MelSpectrogramLoss", mel_loss, 10)]
    cases += [(f"MSE stft scale {w}", lambda f, w=w: stft_loss(f, (w,)), 20) for w in (2048, 512)]
    cases += [(f"MSE mel scale {w} ({m} bands)", lambda f, m=m, w=w: mel_loss(f, (m,), (w,)), 20) for m, w in zip(mels, wins)]
    for name, make, reps in cases:
        losses = {f: make(f) for f in MODES}

        def fn(f):
            xa = xs.clone().requires_grad_(True)
            val = losses[f](A.AudioSignal(xa, 44100), A.AudioSignal(ys, 44100))
            val.backward()
            node = val.grad_fn                     # the first scale's node: the fused Function or torch's own
            while node.name() == "AddBackward0":
                node = next(n for n, _ in node.next_functions if n is not None)
            return xa.grad, node.name()

        outs = {f: fn(f) for f in MODES}           # warm-up of all three paths
        times = {f: [] for f in MODES}
        for _ in range(rounds):
            for f in MODES:
                times[f].append(_timed(lambda: fn(f), reps))
        for f in MODES:
            ts = sorted(times[f])
            diff = float((outs[f][0] - outs[False][0]).abs().max() / outs[False][0].abs().max())
            print(f"{name} fwd + bwd, 32x2chx10s, fused={f}: median {ts[len(ts) // 2]:8.3f} ms  (min {ts[0]:.3f}, max {ts[-1]:.3f}; "
                  f"{rounds} windows of {reps}); {outs[f][1]}; grad rel diff to unfused {diff:.2e}", flush=True)


if CASE in ("all", "mse"):
    run_mse()


def run_wide_mel(rounds=5):
    """The 64-bands-at-every-scale mel recipe (windows 32 ... 2048), forward + backward w.r.t. the estimate: fused=False / True /
    "waveform" alternating in one process, every window between two HIP events; the whole step, then every scale that needs the
    wide kernel (csrc/meldist_wide.hip) alone.  "narrow routing": ``*_supported`` limited to n_mels <= n_fft / 4, i.e. the whole
    step as it ran before the wide kernel existed (those scales unfused, the others fused)."""
    from audiotools_amd import kernels, metrics
    wins = [32, 64, 128, 256, 512, 1024, 2048]
    xs, ys = x[:32], (x[32:64] if B >= 64 else x[:32].flip(0)).clone()
    supported = kernels.mel_distance_supported

    def mel_loss(f, w=wins):
        return metrics.spectral.MelSpectrogramLoss(n_mels=[64] * len(w), window_lengths=list(w), mel_fmin=[0] * len(w),
                                                   mel_fmax=[None] * len(w), pow=1.0, mag_weight=0.0, fused=f)

    def narrow(n_fft, hop, T, n_mels, *rest):
        return n_mels <= n_fft // 4 and supported(n_fft, hop, T, n_mels, *rest)

    cases = [("64-band 7-scale MelSpectrogramLoss", mel_loss, 10, supported), ("the same, narrow routing", mel_loss, 10, narrow)]
    cases += [(f"mel scale {w} (64 bands)", lambda f, w=w: mel_loss(f, (w,)), 20, supported) for w in wins if w < 256]
    for name, make, reps, route in cases:
        losses = {f: make(f) for f in MODES}

        def fn(f):
            xa = xs.clone().requires_grad_(True)
            losses[f](A.AudioSignal(xa, 44100), A.AudioSignal(ys, 44100)).backward()
            return xa.grad

        kernels.mel_distance_supported = route
        try:
            outs = {f: fn(f) for f in MODES}           # warm-up of all three paths
            times = {f: [] for f in MODES}
            for _ in range(rounds):
                for f in MODES:
                    times[f].append(_timed(lambda: fn(f), reps))
        finally:
            kernels.mel_distance_supported = supported
        for f in MODES:
            ts = sorted(times[f])
            diff = float((outs[f] - outs[False]).abs().max() / outs[False].abs().max())
            print(f"{name} fwd + bwd, 32x2chx10s, fused={f}: median {ts[len(ts) // 2]:8.3f} ms  (min {ts[0]:.3f}, max {ts[-1]:.3f}; "
                  f"{rounds} windows of {reps}); grad rel diff to unfused {diff:.2e}", flush=True)


if CASE in ("all", "widemel"):
    run_wide_mel()
