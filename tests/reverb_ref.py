"""The oracle of batched reverberation (jdsp_reverb_batch; not a test module): the definition itself,

    y_u[t] = gain[u] sum_k h[ir[u]][k] x_u[t - k],   0 <= t < len(x_u),   x_u silent before its first sample,

as numpy's DIRECT convolution (np.convolve: dot products, no transform) of the int16 samples with the taps in float64,
times the gain, truncated to the utterance's length.  It shares no FFT with the code under test."""
import numpy as np


def reverb(x, h, gain=1.0):
    """float64 [len(x)]: the utterance x (int16) through the response h (float64 taps) at `gain`"""
    x = np.asarray(x)
    h = np.asarray(h, np.float64).reshape(-1)
    if x.size == 0:
        return np.zeros(0)
    return float(gain) * np.convolve(x.astype(np.float64), h)[:x.size]

