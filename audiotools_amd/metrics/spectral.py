"""Spectral training losses (reference ``audiotools/metrics/spectral.py``).

Each scale calls ``AudioSignal.stft`` / ``mel_spectrogram`` on both signals; for HIP tensors that
require gradients those run the fused forward kernels and their adjoints
(``spectral._NativeStft`` / ``_NativeStftMel``), so a multi-scale mel loss never materialises a
spectrum gradient in HBM.  ``MultiScaleSTFTLoss(fused=True)`` goes further: one kernel per scale takes both signals
to the loss sums and dL/dX (``csrc/stftdist.hip``), no spectrum is written at all; ``MelSpectrogramLoss(fused=True)`` is
the same for the mel distance (``csrc/meldist.hip``; filterbanks with more than window / 4 bands, such as 64 bands at every
scale: ``csrc/meldist_wide.hip``).  ``fused="waveform"`` also keeps dL/dX on chip: the kernel returns the
loss sums and the gradient of the SIGNAL (``csrc/dist_ola.h``), backward is one multiplication.  The fused kernels exist for
two norms: ``loss_fn=nn.L1Loss()`` and ``loss_fn=nn.MSELoss()``."""
import typing

import numpy as np
import torch
from torch import nn

from .. import kernels, tables
from ..spectral import STFTParams


def _scales(window_lengths, match_stride, window_type):
    return [STFTParams(window_length=w, hop_length=w // 4, match_stride=match_stride, window_type=window_type)
            for w in window_lengths]


# loss_fn types the fused distance kernels evaluate (exact types: a subclass may compute anything) -> their ``loss=`` keyword
_FUSED_NORMS = {nn.L1Loss: "l1", nn.MSELoss: "l2"}


def _log_and_linear(loss_fn, a, b, clamp_eps, power, log_weight, mag_weight):
    """log_weight * d(log10 clamp(a)^p, log10 clamp(b)^p) + mag_weight * d(a, b)
    (spectral.py:88-93, 188-193)."""
    la = a.clamp(clamp_eps).pow(power).log10()
    lb = b.clamp(clamp_eps).pow(power).log10()
    return log_weight * loss_fn(la, lb) + mag_weight * loss_fn(a, b)


class _StftDistance(torch.autograd.Function):
    """One scale of the L1 or L2 (``norm``) STFT-magnitude distance as ONE kernel (``kernels.stft_distance``): the value from the two
    signals, and -- only when the estimate needs a gradient -- dL/dX, which backward hands to the native STFT adjoint.
    Neither spectrum nor any intermediate of the loss exists in memory."""

    @staticmethod
    def forward(ctx, est, ref, window, n_fft, hop, clamp_eps, power, log_weight, mag_weight, norm):
        B, C, T = est.shape
        count = B * C * (1 + T // hop) * (n_fft // 2 + 1)
        sums, G = kernels.stft_distance(est.detach(), ref.detach(), window, n_fft, hop, clamp_eps, power,
                                        log_weight / count, mag_weight / count, ctx.needs_input_grad[0], loss=norm)
        ctx.save_for_backward(G, window)
        ctx.cfg = (n_fft, hop, T)
        return (sums[0] * (log_weight / count) + sums[1] * (mag_weight / count)).to(est.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        G, window = ctx.saved_tensors
        n_fft, hop, T = ctx.cfg
        return (kernels.stft_adjoint(G, window, n_fft, hop, T) * grad_out,) + (None,) * 9


class _StftDistanceWave(torch.autograd.Function):
    """:class:`_StftDistance` with the gradient of the signal formed inside the kernel (``kernels.stft_distance_dx``):
    no dL/dX in memory, no adjoint launch, no clone and no fold in backward."""

    @staticmethod
    def forward(ctx, est, ref, window, n_fft, hop, clamp_eps, power, log_weight, mag_weight, norm):
        B, C, T = est.shape
        count = B * C * (1 + T // hop) * (n_fft // 2 + 1)
        args = (est.detach(), ref.detach(), window, n_fft, hop, clamp_eps, power, log_weight / count, mag_weight / count)
        if ctx.needs_input_grad[0]:
            sums, dx = kernels.stft_distance_dx(*args, loss=norm)
            ctx.save_for_backward(dx)
        else:
            sums, _ = kernels.stft_distance(*args, False, loss=norm)
        return (sums[0] * (log_weight / count) + sums[1] * (mag_weight / count)).to(est.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        return (ctx.saved_tensors[0] * grad_out,) + (None,) * 9


class MultiScaleSTFTLoss(nn.Module):
    """Multi-resolution STFT magnitude distance (DDSP, Engel et al. 2019; spectral.py:11-94):
    for every window length w (hop w/4) the log-power and the linear magnitudes are compared with
    ``loss_fn``.  ``weight`` is carried for the trainer, not applied here.

    ``fused=True`` (not in the reference) evaluates every scale that qualifies with the fused distance kernel: both
    signals float32 HIP tensors of one shape, ``loss_fn`` an ``nn.L1Loss`` or an ``nn.MSELoss`` with mean reduction (exactly
    these types; anything else runs unfused), at most one signal requiring
    a gradient, a power-of-two window of 32 ... 2048.  Such a scale does NOT touch ``stft_data`` of either signal; every
    other scale runs the code of ``fused=False``.  ``fused="waveform"``: the same scales, with the gradient of the signal
    from the kernel itself (no spectrum gradient in memory, no adjoint launch)."""

    def __init__(self, window_lengths: typing.List[int] = [2048, 512], loss_fn: typing.Callable = nn.L1Loss(),
                 clamp_eps: float = 1e-5, mag_weight: float = 1.0, log_weight: float = 1.0, pow: float = 2.0,
                 weight: float = 1.0, match_stride: bool = False, window_type: str = None, fused: bool = False):
        super().__init__()
        self.stft_params = _scales(window_lengths, match_stride, window_type)
        self.loss_fn, self.clamp_eps, self.pow = loss_fn, clamp_eps, pow
        self.log_weight, self.mag_weight, self.weight = log_weight, mag_weight, weight
        self.fused = fused

    def _fused_scale(self, x, y, s):
        """The scale's loss from the fused kernel, or None when the scale does not qualify."""
        xa, ya = x.audio_data, y.audio_data
        if not (self.fused and type(self.loss_fn) in _FUSED_NORMS and self.loss_fn.reduction == "mean"
                and xa.is_cuda and ya.is_cuda and xa.dtype == ya.dtype == torch.float32 and xa.ndim == 3
                and xa.shape == ya.shape and xa.device == ya.device):
            return None
        grad = torch.is_grad_enabled()
        gx, gy = grad and xa.requires_grad, grad and ya.requires_grad
        wtype = s.window_type or x.stft_params.window_type
        if (gx and gy) or wtype != (s.window_type or y.stft_params.window_type):
            return None
        supported = kernels.stft_distance_dx_supported if self.fused == "waveform" else kernels.stft_distance_supported
        norm = _FUSED_NORMS[type(self.loss_fn)]
        if not supported(s.window_length, s.hop_length, xa.shape[-1], self.clamp_eps, self.pow, norm):
            return None
        est, ref = (ya, xa) if gy else (xa, ya)          # both norms are symmetric: the signal that needs a gradient is the estimate
        window = x.get_window(wtype, s.window_length, str(xa.device))
        fn = _StftDistanceWave if self.fused == "waveform" else _StftDistance
        return fn.apply(est, ref, window, s.window_length, s.hop_length, float(self.clamp_eps), float(self.pow),
                        float(self.log_weight), float(self.mag_weight), norm)

    def forward(self, x, y):
        total = 0.0
        for s in self.stft_params:
            fused = self._fused_scale(x, y, s)
            if fused is not None:
                total = total + fused
                continue
            # as in the reference, match_stride of the scale is NOT forwarded to stft()
            x.stft(s.window_length, s.hop_length, s.window_type)
            y.stft(s.window_length, s.hop_length, s.window_type)
            total = total + _log_and_linear(self.loss_fn, x.magnitude, y.magnitude, self.clamp_eps, self.pow,
                                            self.log_weight, self.mag_weight)
        return total


class _MelDistance(torch.autograd.Function):
    """One scale of the L1 or L2 (``norm``) mel-spectrogram distance as ONE kernel (``kernels.mel_distance``): the value from the two
    signals, and -- only when the estimate needs a gradient -- dL/dX, which backward hands to the native STFT adjoint.
    Neither spectrum, neither mel tensor nor any intermediate of the loss exists in memory."""

    @staticmethod
    def forward(ctx, est, ref, window, n_fft, hop, mel_tables, n_mels, clamp_eps, power, log_weight, mag_weight, norm):
        B, C, T = est.shape
        count = B * C * (1 + T // hop) * n_mels
        sums, G = kernels.mel_distance(est.detach(), ref.detach(), window, n_fft, hop, mel_tables, n_mels, clamp_eps, power,
                                       log_weight / count, mag_weight / count, ctx.needs_input_grad[0], loss=norm)
        ctx.save_for_backward(G, window)
        ctx.cfg = (n_fft, hop, T)
        return (sums[0] * (log_weight / count) + sums[1] * (mag_weight / count)).to(est.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        G, window = ctx.saved_tensors
        n_fft, hop, T = ctx.cfg
        return (kernels.stft_adjoint(G, window, n_fft, hop, T) * grad_out,) + (None,) * 11


class _MelDistanceWave(torch.autograd.Function):
    """:class:`_MelDistance` with the gradient of the signal formed inside the kernel (``kernels.mel_distance_dx``)."""

    @staticmethod
    def forward(ctx, est, ref, window, n_fft, hop, mel_tables, n_mels, clamp_eps, power, log_weight, mag_weight, norm):
        B, C, T = est.shape
        count = B * C * (1 + T // hop) * n_mels
        args = (est.detach(), ref.detach(), window, n_fft, hop, mel_tables, n_mels, clamp_eps, power, log_weight / count,
                mag_weight / count)
        if ctx.needs_input_grad[0]:
            sums, dx = kernels.mel_distance_dx(*args, loss=norm)
            ctx.save_for_backward(dx)
        else:
            sums, _ = kernels.mel_distance(*args, False, loss=norm)
        return (sums[0] * (log_weight / count) + sums[1] * (mag_weight / count)).to(est.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        return (ctx.saved_tensors[0] * grad_out,) + (None,) * 11


class MelSpectrogramLoss(nn.Module):
    """Multi-resolution mel-spectrogram distance (spectral.py:97-194): scale i uses
    ``n_mels[i]`` bands between ``mel_fmin[i]`` and ``mel_fmax[i]`` on a window of
    ``window_lengths[i]`` (hop = window / 4).

    ``fused=True`` (not in the reference) evaluates every scale that qualifies with the fused mel distance kernel: both
    signals float32 HIP tensors of one shape and sample rate, ``loss_fn`` an ``nn.L1Loss`` or an ``nn.MSELoss`` with mean
    reduction (exactly these types; anything else runs unfused), at most one signal requiring a gradient, a power-of-two window of 32 ... 2048 and at most
    max(window / 4, min(2 window, 512)) bands (above window / 4 the kernel that keeps the target's bands in LDS runs).  Such a scale does NOT
    touch ``stft_data`` of either signal; every other scale runs the code of ``fused=False``.  ``fused="waveform"``: the same
    scales, with the gradient of the signal from the kernel itself."""

    def __init__(self, n_mels: typing.List[int] = [150, 80], window_lengths: typing.List[int] = [2048, 512],
                 loss_fn: typing.Callable = nn.L1Loss(), clamp_eps: float = 1e-5, mag_weight: float = 1.0,
                 log_weight: float = 1.0, pow: float = 2.0, weight: float = 1.0, match_stride: bool = False,
                 mel_fmin: typing.List[float] = [0.0, 0.0], mel_fmax: typing.List[float] = [None, None],
                 window_type: str = None, fused: bool = False):
        super().__init__()
        self.stft_params = _scales(window_lengths, match_stride, window_type)
        self.n_mels, self.mel_fmin, self.mel_fmax = n_mels, mel_fmin, mel_fmax
        self.loss_fn, self.clamp_eps, self.pow = loss_fn, clamp_eps, pow
        self.log_weight, self.mag_weight, self.weight = log_weight, mag_weight, weight
        self.fused = fused

    def _fused_scale(self, x, y, s, n_mels, fmin, fmax):
        """The scale's loss from the fused kernel, or None when the scale does not qualify."""
        xa, ya = x.audio_data, y.audio_data
        if not (self.fused and type(self.loss_fn) in _FUSED_NORMS and self.loss_fn.reduction == "mean"
                and xa.is_cuda and ya.is_cuda and xa.dtype == ya.dtype == torch.float32 and xa.ndim == 3
                and xa.shape == ya.shape and xa.device == ya.device and x.sample_rate == y.sample_rate):
            return None
        grad = torch.is_grad_enabled()
        gx, gy = grad and xa.requires_grad, grad and ya.requires_grad
        wtype = s.window_type or x.stft_params.window_type
        if (gx and gy) or wtype != (s.window_type or y.stft_params.window_type):
            return None
        supported = kernels.mel_distance_dx_supported if self.fused == "waveform" else kernels.mel_distance_supported
        norm = _FUSED_NORMS[type(self.loss_fn)]
        if not supported(s.window_length, s.hop_length, xa.shape[-1], n_mels, self.clamp_eps, self.pow, norm):
            return None
        mel_tables = tables.mel_dist_tables(x.sample_rate, s.window_length, n_mels, fmin, fmax, xa.device)
        if mel_tables is None:
            return None
        est, ref = (ya, xa) if gy else (xa, ya)          # both norms are symmetric: the signal that needs a gradient is the estimate
        window = x.get_window(wtype, s.window_length, str(xa.device))
        fn = _MelDistanceWave if self.fused == "waveform" else _MelDistance
        return fn.apply(est, ref, window, s.window_length, s.hop_length, mel_tables, n_mels, float(self.clamp_eps),
                        float(self.pow), float(self.log_weight), float(self.mag_weight), norm)

    def forward(self, x, y):
        total = 0.0
        for n_mels, fmin, fmax, s in zip(self.n_mels, self.mel_fmin, self.mel_fmax, self.stft_params):
            fused = self._fused_scale(x, y, s, n_mels, fmin, fmax) if self.fused else None
            if fused is not None:
                total = total + fused
                continue
            kw = dict(window_length=s.window_length, hop_length=s.hop_length, window_type=s.window_type)
            mx = x.mel_spectrogram(n_mels, mel_fmin=fmin, mel_fmax=fmax, **kw)
            my = y.mel_spectrogram(n_mels, mel_fmin=fmin, mel_fmax=fmax, **kw)
            total = total + _log_and_linear(self.loss_fn, mx, my, self.clamp_eps, self.pow, self.log_weight,
                                            self.mag_weight)
        return total


class PhaseLoss(nn.Module):
    """Magnitude-weighted squared phase difference (spectral.py:197-247).

    Bug-compatible with the reference's wrap-around: differences below -pi get +2 pi, differences
    above +pi ALSO get +2 pi (the reference subtracts a negative), so only one side is wrapped."""

    def __init__(self, window_length: int = 2048, hop_length: int = 512, weight: float = 1.0):
        super().__init__()
        self.weight = weight
        self.stft_params = STFTParams(window_length, hop_length)

    def forward(self, x, y):
        s = self.stft_params
        x.stft(s.window_length, s.hop_length, s.window_type)
        y.stft(s.window_length, s.hop_length, s.window_type)
        diff = x.phase - y.phase
        diff[diff < -np.pi] += 2 * np.pi
        diff[diff > np.pi] += 2 * np.pi
        mag = x.magnitude
        lo, hi = mag.min(), mag.max()
        weights = (mag - lo) / (hi - lo)
        return ((weights * diff) ** 2).mean()
