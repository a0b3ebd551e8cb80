"""Python mirror of the C ABI: one Engine == one jdsp_ctx.

Host arrays (numpy) go through the host entry points (copy in, run, copy out);
torch CUDA tensors go through the *_dev entry points on torch's current stream,
so torch.cuda.Event timing and stream ordering see the kernels.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import JdspError

L = _lib.lib


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _batch_offsets(holder, key, sample_first, unit_first, dev):
    """The offsets of the last batch stay on the device: the device copies of the two int64 host arrays, made anew when
    (key, dev) differs from the last call's and kept on `holder` -- the Engine or the stream object itself, so the
    batch entries of two objects never share a cache.  Returns (d_sample, d_unit, fresh)."""
    fresh = getattr(holder, "_batch_key", None) != (key, dev)
    if fresh:
        import torch
        holder._batch_dev = (torch.from_numpy(sample_first).to(dev), torch.from_numpy(unit_first).to(dev))
        holder._batch_key = (key, dev)
    return holder._batch_dev + (fresh,)


def _batch_out(n, dtype, dev, given=None, tail=()):
    """One output buffer of a batch entry: `given` as it is, else zeros [max(n, 1), *tail] of the numpy dtype `dtype`,
    on the torch device dev or, with dev None, in numpy."""
    if given is not None:
        return given
    shape = (max(n, 1),) + tuple(tail)
    if dev is None:
        return np.zeros(shape, dtype)
    import torch
    return torch.zeros(shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)


class _Handle:
    """Owns one C handle in `_h`: closed when collected."""

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Child(_Handle):
    """A stream object of an Engine; `_destroy` is its jdsp_*_destroy."""
    _destroy = None

    def close(self):
        if getattr(self, "_h", None):
            type(self)._destroy(self._h)
            self._h = None
            if self in self.eng._children:
                self.eng._children.remove(self)


class Engine(_Handle):
    def __init__(self, device=0):
        h = C.c_void_p()
        rc = L.jdsp_create(int(device), C.byref(h))
        if rc != 0:
            raise JdspError(rc, L.jdsp_last_error(None).decode())
        self._h = h
        self._children = []           # stream objects that hold a pointer to this ctx: destroyed first
        self.device = int(device)
        n_cu, hbm = C.c_int(), C.c_size_t()
        name = C.create_string_buffer(96)
        self._ck(L.jdsp_device_info(h, C.byref(n_cu), C.byref(hbm), name, 96))
        self.n_cu, self.hbm_bytes, self.name = n_cu.value, hbm.value, name.value.decode()

    def close(self):
        if getattr(self, "_h", None):
            for c in list(self._children):
                c.close()
            L.jdsp_destroy(self._h)
            self._h = None

    def _ck(self, rc):
        if rc != 0:
            raise JdspError(rc, L.jdsp_last_error(self._h).decode())

    def _use_torch_stream(self):
        import torch
        self._ck(L.jdsp_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def set_option(self, name, value):
        self._ck(L.jdsp_set_option(self._h, name.encode(), int(value)))

    def fastconv(self, taps, n_fft):
        return FastConv(self, taps, n_fft)

    def reverb(self, taps):
        """Batched reverberator (jdsp_reverb) over the bank taps [n_irs, n_taps] of impulse responses."""
        return Reverb(self, taps)

    def binaural(self, hrirs):
        """Live binaural renderer (jdsp_binaural) over the bank hrirs [n_dirs, 2, n_taps]."""
        return Binaural(self, hrirs)

    def mvdr_multi(self, n_mics, delays=None, loading=0.0, n_fft=1024):
        return MvdrMulti(self, n_mics, delays, loading, n_fft)

    def mvdr(self, d_time=0.0):
        return Mvdr(self, d_time)

    def mfcc(self, **cfg):
        return Mfcc(self, **cfg)

    def gmm(self, classes):
        return Gmm(self, classes)

    def hmm(self, models):
        return Hmm(self, models)

    def gmm_trainer(self, n_classes):
        """GMM training (jdsp_gmm_trainer) of n_classes classes (1..1024), GMMAlgorithm_Train_Auto_ver2.cpp."""
        return GmmTrainer(self, n_classes)

    def denoiser(self, mode, n_fft=1024, hop=512):
        return Denoiser(self, mode, n_fft, hop)

    def istft(self, **cfg):
        """STFT synthesis stream (jdsp_istft): n_fft, hop, layout ("full" / "half" or 0 / 1), synthesis_window,
        analysis_window ("none" / "hamming" / "hann" or -1 / 0 / 1)."""
        return Istft(self, **cfg)

    def stft_mask(self, **cfg):
        """Fused STFT masking stream (jdsp_stftmask): n_fft, hop, analysis_window, synthesis_window ("none" /
        "hamming" / "hann" or -1 / 0 / 1), normalise (0 / 1), mask_kind ("real" / "complex" or 0 / 1)."""
        return StftMask(self, **cfg)

    def geq(self, n_streams, coeff=None):
        """Multi-stream IIR equaliser (jdsp_geq), 7Band_GEQ.cpp: coeff [n_sections, 2, 3] float64 (1..16 sections), or
        None for the reference's seven bands (geq_design())."""
        return Geq(self, n_streams, coeff)

    def nlms(self, n_streams, filter_len=256, mu=1e-4, compensation=1e-4):
        """Multi-stream normalised LMS filter (jdsp_nlms), NormalLMS.cpp: filter_len 64 | 128 | 256."""
        return Nlms(self, n_streams, filter_len, mu, compensation)

    def synchronize(self):
        self._ck(L.jdsp_synchronize(self._h))

    # ---- VoiceActivityDetection on its own (SS:121-156 = WF:261-296; BF:207-242) ----
    def vad_blocks(self, blocks, variant="denoise"):
        """blocks int16 [n, 512 | 256] (host) -> (voice uint8 [n], energy sums int64 [n], zero crossings int32 [n]).
        variant "denoise": energy > 700 or ZCR < 200; "mvdr": BeamForming_MVDR_ver1.cpp's frame offset, energy only."""
        blocks = np.ascontiguousarray(np.atleast_2d(blocks), np.int16)
        n, bl = blocks.shape
        v = np.zeros(n, np.uint8)
        e = np.zeros(n, np.int64)
        z = np.zeros(n, np.int32)
        self._ck(L.jdsp_vad_blocks_ex(self._h, {"denoise": 0, "mvdr": 1}[variant], bl, _vp(blocks), n, _vp(v), _vp(e), _vp(z)))
        return v, e, z

    # ---- FFTAlgorithm_ver2.cpp ------------------------------------------------
    def bitrev_table(self, n_fft, block_len=None):
        """Bitrev table (FFTAlgorithm_ver2.cpp:186-202) computed on the device; int16[n_fft]."""
        t = np.zeros(n_fft, np.int16)
        self._ck(L.jdsp_bitrev_table(self._h, n_fft, block_len or n_fft, t.ctypes.data_as(C.c_void_p)))
        return t

    def fft_process(self, x, forward=True):
        """Batched FFTProcess (FFTAlgorithm_ver2.cpp:94-149): complex128 [..., n_fft], unnormalised."""
        if _is_torch(x):
            import torch
            assert x.is_cuda and x.dtype == torch.complex128 and x.is_contiguous()
            out = torch.empty_like(x)
            n = x.shape[-1]
            self._use_torch_stream()
            self._ck(L.jdsp_fft_process_f64_dev(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), n,
                                                x.numel() // n, int(forward)))
            return out
        x = np.ascontiguousarray(x, np.complex128)
        out = np.empty_like(x)
        n = x.shape[-1]
        self._ck(L.jdsp_fft_process_f64(self._h, x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), n,
                                        x.size // n, int(forward)))
        return out

    DFT_I16, IDFT, IDFT_OVER_N = 0, 1, 2

    def dft_direct(self, kind, x, accumulate_into=None):
        """DFTProcess / IDFTProcess / IFFTProcess (FFTAlgorithm_ver2.cpp:162-173 / :175-184 / :151-160): the
        O(N^2) sums as the reference writes them, any length, ADDED to `accumulate_into` (default: zeros).
        x: int16 [..., n] for DFT_I16, complex128 [..., n] otherwise.  Returns complex128 [..., n]."""
        x = np.ascontiguousarray(x, np.int16 if kind == self.DFT_I16 else np.complex128)
        n = x.shape[-1]
        out = np.zeros(x.shape, np.complex128) if accumulate_into is None else \
            np.ascontiguousarray(accumulate_into, np.complex128).copy()
        assert out.shape == x.shape
        self._ck(L.jdsp_dft_direct_f64(self._h, int(kind), x.ctypes.data_as(C.c_void_p),
                                       out.ctypes.data_as(C.c_void_p), n, x.size // n))
        return out

    def gmm_probability(self, feats, mean, cov, eig):
        """probability() (GMMAlgorithm_Test_Auto_ver2.cpp:164-236) of every 12-double vector of feats under one
        mixture component (mean [12], cov [12, 12], eig [12, 4])."""
        feats = np.ascontiguousarray(np.atleast_2d(feats), np.float64)
        mean = np.ascontiguousarray(mean, np.float64)
        cov = np.ascontiguousarray(cov, np.float64)
        eig = np.ascontiguousarray(eig, np.float64)
        assert feats.shape[1] == 12 and mean.size == 12 and cov.size == 144 and eig.size == 48
        out = np.empty(feats.shape[0], np.float64)
        self._ck(L.jdsp_gmm_probability(self._h, _vp(feats), feats.shape[0], _vp(mean), _vp(cov), _vp(eig), _vp(out)))
        return out

    # ---- PitchEstimation_method1.cpp ---------------------------------------------
    def pitch(self, pcm, prev_block=None, want_autocorr=False):
        """CalcPitch (PitchEstimation_method1.cpp:69-116) for every 512-sample block of pcm:
        returns (arg int32[nb], rmax float32[nb][, autocorr float32[nb,512]])."""
        if _is_torch(pcm):
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous() and pcm.numel() % 512 == 0
            nb = pcm.numel() // 512
            arg = torch.empty(nb, dtype=torch.int32, device=pcm.device)
            rmax = torch.empty(nb, dtype=torch.float32, device=pcm.device)
            ac = torch.empty((nb, 512), dtype=torch.float32, device=pcm.device) if want_autocorr else None
            self._use_torch_stream()
            self._ck(L.jdsp_pitch_autocorr_dev(self._h, C.c_void_p(pcm.data_ptr()), nb,
                                               C.c_void_p(prev_block.data_ptr()) if prev_block is not None else None,
                                               C.c_void_p(arg.data_ptr()), C.c_void_p(rmax.data_ptr()),
                                               C.c_void_p(ac.data_ptr()) if want_autocorr else None))
            return (arg, rmax, ac) if want_autocorr else (arg, rmax)
        pcm = np.ascontiguousarray(pcm, np.int16)
        assert pcm.size % 512 == 0
        nb = pcm.size // 512
        arg = np.zeros(nb, np.int32)
        rmax = np.zeros(nb, np.float32)
        ac = np.zeros((nb, 512), np.float32) if want_autocorr else None
        pb = np.ascontiguousarray(prev_block, np.int16) if prev_block is not None else None
        self._ck(L.jdsp_pitch_autocorr(self._h, pcm.ctypes.data_as(C.c_void_p), nb,
                                       pb.ctypes.data_as(C.c_void_p) if pb is not None else None,
                                       arg.ctypes.data_as(C.c_void_p), rmax.ctypes.data_as(C.c_void_p),
                                       ac.ctypes.data_as(C.c_void_p) if want_autocorr else None))
        return (arg, rmax, ac) if want_autocorr else (arg, rmax)

    # ---- PitchEstimation_method2.cpp / PitchEstimation_method3.cpp ---------------------
    def pitch_lag(self, pcm, method, prev_block=None, want_curve=False):
        """CalcPitch of PitchEstimation_method2.cpp (method 2, AMDF: arg min) or _method3.cpp (method 3, time-domain
        autocorrelation: arg max), :69-101, for every 512-sample block of pcm, bit-exact:
        returns (arg int32[nb], value float64[nb][, curve float64[nb,512]])."""
        method = int(method)
        if _is_torch(pcm):
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous() and pcm.numel() % 512 == 0
            nb = pcm.numel() // 512
            arg = torch.empty(nb, dtype=torch.int32, device=pcm.device)
            val = torch.empty(nb, dtype=torch.float64, device=pcm.device)
            cv = torch.empty((nb, 512), dtype=torch.float64, device=pcm.device) if want_curve else None
            self._use_torch_stream()
            self._ck(L.jdsp_pitch_lag_dev(self._h, method, C.c_void_p(pcm.data_ptr()), nb,
                                          C.c_void_p(prev_block.data_ptr()) if prev_block is not None else None,
                                          C.c_void_p(arg.data_ptr()), C.c_void_p(val.data_ptr()),
                                          C.c_void_p(cv.data_ptr()) if want_curve else None))
            return (arg, val, cv) if want_curve else (arg, val)
        pcm = np.ascontiguousarray(pcm, np.int16)
        assert pcm.size % 512 == 0
        nb = pcm.size // 512
        arg = np.zeros(nb, np.int32)
        val = np.zeros(nb, np.float64)
        cv = np.zeros((nb, 512), np.float64) if want_curve else None
        pb = np.ascontiguousarray(prev_block, np.int16) if prev_block is not None else None
        assert pb is None or pb.size == 512
        self._ck(L.jdsp_pitch_lag(self._h, method, _vp(pcm), nb, _vp(pb) if pb is not None else None, _vp(arg), _vp(val),
                                  _vp(cv) if want_curve else None))
        return (arg, val, cv) if want_curve else (arg, val)

    # ---- LPCEstimation.cpp -------------------------------------------------------------
    def lpc(self, pcm, block_len=256, order=12, prev_block=None, want_autocorr=False):
        """LPCEstimation (LPCEstimation.cpp:87-137) for every block_len-sample block of pcm (256 | 512), order 1..16:
        returns lpc float64[nb, order] (every block gets a vector, the stream's first included), with
        want_autocorr (lpc, autocorr float64[nb, order + 1]).  An all-zero frame gives NaNs."""
        block_len, order = int(block_len), int(order)
        if _is_torch(pcm):
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
            assert block_len > 0 and pcm.numel() % block_len == 0
            nb = pcm.numel() // block_len
            out = torch.empty((nb, max(order, 0)), dtype=torch.float64, device=pcm.device)
            ac = torch.empty((nb, max(order, 0) + 1), dtype=torch.float64, device=pcm.device) if want_autocorr else None
            self._use_torch_stream()
            self._ck(L.jdsp_lpc_dev(self._h, C.c_void_p(pcm.data_ptr()), nb, block_len, order,
                                    C.c_void_p(prev_block.data_ptr()) if prev_block is not None else None,
                                    C.c_void_p(ac.data_ptr()) if want_autocorr else None, C.c_void_p(out.data_ptr())))
            return (out, ac) if want_autocorr else out
        pcm = np.ascontiguousarray(pcm, np.int16)
        assert block_len > 0 and pcm.size % block_len == 0
        nb = pcm.size // block_len
        out = np.zeros((nb, max(order, 0)), np.float64)
        ac = np.zeros((nb, max(order, 0) + 1), np.float64) if want_autocorr else None
        pb = np.ascontiguousarray(prev_block, np.int16) if prev_block is not None else None
        assert pb is None or pb.size == block_len
        self._ck(L.jdsp_lpc(self._h, _vp(pcm), nb, block_len, order, _vp(pb) if pb is not None else None,
                            _vp(ac) if want_autocorr else None, _vp(out)))
        return (out, ac) if want_autocorr else out

    def stft_half(self, pcm, n_frames=None, out=None, pitch=513):
        """Bins 0..512 only: complex64 [n_frames, pitch >= 513], columns past 512 untouched."""
        import torch
        assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
        if n_frames is None:
            n_frames = (pcm.numel() - 1024) // 512 + 1 if pcm.numel() >= 1024 else 0
        if out is None:
            out = torch.empty((n_frames, pitch), dtype=torch.complex64, device=pcm.device)
        assert out.is_contiguous() and out.shape[-1] == pitch
        self._use_torch_stream()
        self._ck(L.jdsp_stft_half_i16_dev(self._h, C.c_void_p(pcm.data_ptr()), n_frames, C.c_void_p(out.data_ptr()),
                                          pitch))
        return out

    def stft_half_batch(self, pcm, utt_sample_first, hop=512, pitch=520, out=None):
        """Bins 0..512 of every frame of a batch of ragged utterances in one launch (jdsp_stft_half_batch): pcm is
        int16 with the utterances packed at the n_utts + 1 even sample offsets utt_sample_first (a host sequence;
        sharding.stftmask_batch_layout gives each utterance's frame count F_u and first row).  Returns complex64
        [sum F_u, pitch]: row frame_first[u] + f equals Engine.stft(pcm_u, F_u, 1024, hop)[f, :513] bit for bit;
        columns past 512 are untouched.  pitch must be even and >= 514.  hop 1024, 512 or 256; window by
        "stft.window".  torch CUDA input (the device entry on torch's current stream) or numpy (the host entry)."""
        from .sharding import stftmask_batch_layout
        offs = np.ascontiguousarray(utt_sample_first, np.int64).reshape(-1)
        counts, frame_first = stftmask_batch_layout(offs, 1024, hop)
        n_utts, n_total, n_samples = counts.size, int(frame_first[-1]), int(pcm.shape[0])
        assert pcm.ndim == 1 and n_samples >= int(offs[-1])
        sample_first = np.ascontiguousarray(offs[:-1])
        if _is_torch(pcm):
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
            dev = pcm.device
            d_sample, d_frame, _ = _batch_offsets(self, (offs.tobytes(), hop), sample_first, frame_first, dev)
            if out is None:
                out = torch.empty((n_total, pitch), dtype=torch.complex64, device=dev)
            assert out.is_cuda and out.dtype == torch.complex64 and out.is_contiguous()
            assert out.ndim == 2 and out.shape[0] >= n_total and out.shape[1] == pitch
            self._use_torch_stream()
            self._ck(L.jdsp_stft_half_batch_dev(self._h, _vp(pcm), _vp(d_sample), _vp(d_frame), n_utts, n_total, int(hop),
                                                _vp(out), int(pitch)))
        else:
            pcm = np.ascontiguousarray(pcm, np.int16)
            if out is None:
                out = np.zeros((n_total, pitch), np.complex64)
            assert out.dtype == np.complex64 and out.flags.c_contiguous
            assert out.ndim == 2 and out.shape[0] >= n_total and out.shape[1] == pitch
            self._ck(L.jdsp_stft_half_batch(self._h, _vp(pcm), n_samples, _vp(sample_first), _vp(frame_first), n_utts,
                                            int(hop), _vp(out), int(pitch)))
        return out[:n_total]

    # ---- STFT analysis (SS:218-230 / WF:181-193 for a whole batch) ---------
    def stft(self, pcm, n_frames=None, n_fft=1024, hop=512, out=None):
        """pcm: int16 numpy array (host path) or torch CUDA int16 tensor (device path).
        Returns complex64 [n_frames, n_fft]."""
        if _is_torch(pcm):
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
            total = pcm.numel()
            if n_frames is None:
                n_frames = (total - n_fft) // hop + 1 if total >= n_fft else 0
            assert n_frames == 0 or hop * (n_frames - 1) + n_fft <= total, "pcm too short"
            if out is None:
                out = torch.empty((n_frames, n_fft), dtype=torch.complex64, device=pcm.device)
            assert out.is_contiguous() and out.dtype == torch.complex64 and out.numel() >= n_frames * n_fft
            self._use_torch_stream()
            self._ck(L.jdsp_stft_i16_dev(self._h, C.c_void_p(pcm.data_ptr()), n_frames, n_fft, hop,
                                         C.c_void_p(out.data_ptr())))
            return out
        pcm = np.ascontiguousarray(pcm, np.int16)
        nf = C.c_long()
        total = pcm.size
        want = (total - n_fft) // hop + 1 if total >= n_fft else 0
        if out is not None:              # e.g. a pinned buffer: the library then pipelines the PCIe copies
            res = out
            assert res.dtype == np.complex64 and res.flags.c_contiguous and res.shape == (max(want, 0), n_fft)
        else:
            res = np.empty((max(want, 0), n_fft), np.complex64)
        self._ck(L.jdsp_stft_i16(self._h, pcm.ctypes.data_as(C.c_void_p), total, n_fft, hop,
                                 res.ctypes.data_as(C.c_void_p), C.byref(nf)))
        assert nf.value == want
        return res

    def stft_f64(self, pcm, n_frames=None, hop=512, out=None):
        """The 1024-point analysis in FP64 (jdsp_stft_i16_f64*): complex128 [n_frames, 1024]."""
        n_fft = 1024
        if _is_torch(pcm):
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
            total = pcm.numel()
            if n_frames is None:
                n_frames = (total - n_fft) // hop + 1 if total >= n_fft else 0
            assert n_frames == 0 or hop * (n_frames - 1) + n_fft <= total, "pcm too short"
            if out is None:
                out = torch.empty((n_frames, n_fft), dtype=torch.complex128, device=pcm.device)
            assert out.is_contiguous() and out.dtype == torch.complex128 and out.numel() >= n_frames * n_fft
            self._use_torch_stream()
            self._ck(L.jdsp_stft_i16_f64_dev(self._h, C.c_void_p(pcm.data_ptr()), n_frames, n_fft, hop,
                                             C.c_void_p(out.data_ptr())))
            return out
        pcm = np.ascontiguousarray(pcm, np.int16)
        nf = C.c_long()
        want = (pcm.size - n_fft) // hop + 1 if pcm.size >= n_fft else 0
        res = np.empty((max(want, 0), n_fft), np.complex128)
        self._ck(L.jdsp_stft_i16_f64(self._h, pcm.ctypes.data_as(C.c_void_p), pcm.size, n_fft, hop,
                                     res.ctypes.data_as(C.c_void_p), C.byref(nf)))
        assert nf.value == want
        return res


class Denoiser(_Child):
    """One SS/Wiener audio stream (jdsp_denoise): mirrors main()'s loop of
    SpectralSubtraction_final.cpp:92-113 / WienerFilter_final.cpp:91-112 for batches of blocks."""
    _destroy = staticmethod(lambda h: L.jdsp_denoise_destroy(h))
    SPECSUB, WIENER = 0, 1

    def __init__(self, engine, mode, n_fft=1024, hop=512):
        self.eng = engine
        h = C.c_void_p()
        engine._ck(L.jdsp_denoise_create_cfg(engine._h, int(mode), int(n_fft), int(hop), C.byref(h)))
        self._h = h
        self.n_fft, self.block = int(n_fft), L.jdsp_denoise_block_len(h)
        engine._children.append(self)

    def reset(self):
        self.eng._ck(L.jdsp_denoise_reset(self._h))

    def set_option(self, name, value):
        self.eng._ck(L.jdsp_denoise_set_option(self._h, name.encode(), int(value)))

    def blocks_out(self, n_blocks):
        return L.jdsp_denoise_blocks_out(self._h, n_blocks)

    def process(self, pcm, want_precast=False):
        """pcm: int16, a whole number of blocks (self.block samples: 512, or 256 for 512-point frames).
        numpy -> host path, torch CUDA -> device path.  Returns out (int16) or (out, precast float32)."""
        B = self.block
        if _is_torch(pcm):
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous() and pcm.numel() % B == 0
            nb = pcm.numel() // B
            n_out = self.blocks_out(nb)
            out = torch.empty(max(n_out, 1) * B, dtype=torch.int16, device=pcm.device)
            pre = torch.empty(max(n_out, 1) * B, dtype=torch.float32, device=pcm.device) if want_precast else None
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_denoise_process_dev(self._h, C.c_void_p(pcm.data_ptr()), nb, C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(pre.data_ptr()) if want_precast else None, None))
            out = out[:n_out * B]
            return (out, pre[:n_out * B]) if want_precast else out
        pcm = np.ascontiguousarray(pcm, np.int16)
        assert pcm.size % B == 0
        nb = pcm.size // B
        n_out = self.blocks_out(nb)
        out = np.zeros(max(n_out, 1) * B, np.int16)
        pre = np.zeros(max(n_out, 1) * B, np.float32) if want_precast else None
        got = C.c_long()
        self.eng._ck(L.jdsp_denoise_process(self._h, pcm.ctypes.data_as(C.c_void_p), nb, out.ctypes.data_as(C.c_void_p),
                                            pre.ctypes.data_as(C.c_void_p) if want_precast else None, C.byref(got)))
        assert got.value == n_out
        return (out[:n_out * B], pre[:n_out * B]) if want_precast else out[:n_out * B]

    def reserve_batch(self, max_blocks_total, max_utts):
        """Sizes the workspace of process_batch's device path (jdsp_denoise_batch_reserve): the only call of the batch
        entries that allocates.  Call it before capturing process_batch in a graph."""
        self.eng._ck(L.jdsp_denoise_batch_reserve(self._h, int(max_blocks_total), int(max_utts)))

    def process_batch(self, pcm, block_counts, utt_sample_first=None, want_precast=False, want_flags=False,
                      want_noise=False, out=None):
        """A batch of independent utterances in one launch sequence (jdsp_denoise_batch): each comes out as a fresh
        handle's process of its blocks, and the handle's own stream is neither read nor advanced.  (1024, 512) handles.
        pcm: int16; block_counts: B_u >= 0 blocks of self.block samples per utterance (a host sequence);
        utt_sample_first: the n_utts even sample offsets of the spans, ascending and disjoint (None: packed back to
        back, sharding.denoise_batch_layout).  torch CUDA (the device entry on torch's current stream; it reserves on
        demand, so call reserve_batch first under graph capture) or numpy (the host entry).  Returns int16 of pcm's
        length, TIME-ALIGNED with pcm: the enhanced samples of utterance u's blocks 1 .. B_u - 2 lie where those blocks
        lie in pcm; everything else is zero, or is left as it was in `out` when given on the device path.  With
        want_precast / want_flags / want_noise a tuple follows the same order: float32 samples before the cast, uint8
        VAD decisions [sum B_u] in concatenated block order, float32 [n_utts, 1024] estimates in force after each
        utterance's last block."""
        from .sharding import denoise_batch_layout
        counts = np.ascontiguousarray(block_counts, np.int64).reshape(-1)
        packed, block_first, n_packed = denoise_batch_layout(counts, self.block)
        if utt_sample_first is None:
            sample_first = packed
        else:
            sample_first = np.ascontiguousarray(utt_sample_first, np.int64).reshape(-1)[:counts.size]
            assert sample_first.size == counts.size
        n_utts, n_total, n_samples = counts.size, int(block_first[-1]), int(pcm.shape[0])
        assert pcm.ndim == 1
        dev = pcm.device if _is_torch(pcm) else None
        if dev is not None:
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
            assert n_utts == 0 or int((sample_first + counts * self.block).max()) <= n_samples
            key = (sample_first.tobytes(), counts.tobytes())
            d_sample, d_block, fresh = _batch_offsets(self, key, sample_first, block_first, dev)
            if fresh:
                self.reserve_batch(n_total, n_utts)             # a no-op once sized
        else:
            pcm = np.ascontiguousarray(pcm, np.int16)
        out = _batch_out(n_samples, np.int16, dev, out)
        pre = _batch_out(n_samples, np.float32, dev) if want_precast else None
        flags = _batch_out(n_total, np.uint8, dev) if want_flags else None
        noise = _batch_out(n_utts, np.float32, dev, tail=(1024,)) if want_noise else None
        if dev is not None:
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_denoise_batch_dev(self._h, _vp(pcm), _vp(d_sample), _vp(d_block), n_utts, n_total, _vp(out),
                                                  _vp(pre), _vp(flags), _vp(noise)))
        else:
            self.eng._ck(L.jdsp_denoise_batch(self._h, _vp(pcm), n_samples, _vp(sample_first), _vp(block_first), n_utts,
                                              _vp(out), _vp(pre), _vp(flags), _vp(noise)))
        res = [out[:n_samples]]
        if want_precast:
            res.append(pre[:n_samples])
        if want_flags:
            res.append(flags[:n_total])
        if want_noise:
            res.append(noise[:n_utts])
        return res[0] if len(res) == 1 else tuple(res)

    # ---- live streams: n independent streams in the handle, advanced a chunk each by one call (jdsp_denoise_streams_*)
    def open_streams(self, n_streams, max_blocks_total):
        """Gives the handle n_streams live streams, all fresh, and the workspace of calls of up to max_blocks_total
        blocks (jdsp_denoise_streams_reserve): the only call of the live entries that allocates, and it synchronises.
        Calling it again discards every live stream's state."""
        self.eng._ck(L.jdsp_denoise_streams_reserve(self._h, int(n_streams), int(max_blocks_total)))
        self.n_streams = int(n_streams)
        self._streams_torch = None      # the kind of the last process_streams() input
        self._streams_key = None

    def process_streams(self, pcm, stream_ids, block_counts, chunk_sample_first=None, want_precast=False,
                        want_flags=False):
        """One call over live streams (jdsp_denoise_streams; open_streams first): chunk c continues the live stream
        stream_ids[c] with block_counts[c] >= 0 NEW blocks of self.block samples, at chunk_sample_first[c] of pcm (even,
        ascending, disjoint; None: back to back, sharding.denoise_batch_layout).  Ids are distinct within a call.  The
        chunk's E_c emitted blocks (sharding.denoise_stream_emitted) come out PACKED from the span's start; a stream's
        emitted blocks over its calls equal, bit for bit, process_batch of all its blocks as one utterance.  torch CUDA
        (the device entry on torch's current stream) or numpy (the host entry).  Returns (out int16 of pcm's length
        [, precast float32][, flags uint8 [sum B_c]], n_emitted int64 [n_chunks]); what no chunk emitted is zero."""
        from .sharding import denoise_batch_layout
        ids = np.ascontiguousarray(stream_ids, np.int64).reshape(-1)
        counts = np.ascontiguousarray(block_counts, np.int64).reshape(-1)
        assert ids.size == counts.size, "one block count per chunk"
        packed, block_first, _ = denoise_batch_layout(counts, self.block)
        if chunk_sample_first is None:
            sample_first = packed
        else:
            sample_first = np.ascontiguousarray(chunk_sample_first, np.int64).reshape(-1)
            assert sample_first.size == ids.size
        n_chunks, n_total, n_samples = ids.size, int(block_first[-1]), int(pcm.shape[0])
        assert pcm.ndim == 1
        dev = pcm.device if _is_torch(pcm) else None
        self._streams_torch = dev
        if dev is not None:
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
            assert n_chunks == 0 or int((sample_first + counts * self.block).max()) <= n_samples
            key = (ids.tobytes(), sample_first.tobytes(), counts.tobytes(), dev)
            if self._streams_key != key:
                self._streams_dev = tuple(torch.from_numpy(a).to(dev) for a in (ids, sample_first, block_first))
                self._streams_key = key
            d_ids, d_sample, d_block = self._streams_dev
        else:
            pcm = np.ascontiguousarray(pcm, np.int16)
        out = _batch_out(n_samples, np.int16, dev)
        pre = _batch_out(n_samples, np.float32, dev) if want_precast else None
        flags = _batch_out(n_total, np.uint8, dev) if want_flags else None
        emitted = _batch_out(n_chunks, np.int64, dev)
        if dev is not None:
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_denoise_streams_dev(self._h, _vp(pcm), _vp(d_ids), _vp(d_sample), _vp(d_block), n_chunks,
                                                    n_total, _vp(out), _vp(pre), _vp(flags), _vp(emitted)))
        else:
            self.eng._ck(L.jdsp_denoise_streams(self._h, _vp(pcm), n_samples, _vp(ids), _vp(sample_first), _vp(block_first),
                                                n_chunks, _vp(out), _vp(pre), _vp(flags), _vp(emitted)))
        res = [out[:n_samples]]
        if want_precast:
            res.append(pre[:n_samples])
        if want_flags:
            res.append(flags[:n_total])
        res.append(emitted[:n_chunks])
        return tuple(res)

    def reset_streams(self, stream_ids=None):
        """The listed live streams fresh again, or all of them with None (jdsp_denoise_streams_reset_dev; enqueue-only)."""
        if stream_ids is None:
            if self._streams_torch is not None:
                self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_denoise_streams_reset_dev(self._h, None, 0))
            return
        import torch
        ids = np.ascontiguousarray(stream_ids, np.int64).reshape(-1)
        dev = self._streams_torch if self._streams_torch is not None else torch.device("cuda", self.eng.device)
        d_ids = torch.from_numpy(ids).to(dev)
        self.eng._use_torch_stream()
        self.eng._ck(L.jdsp_denoise_streams_reset_dev(self._h, _vp(d_ids), ids.size))
        self._reset_args = d_ids                                # alive until the stream has run the call

    def streams_state(self, stream_ids):
        """(estimates float32 [n_ids, 1024] in process_batch's want_noise layout, zeros where nothing has latched;
        blocks seen int64 [n_ids]) of the listed live streams (jdsp_denoise_streams_state; synchronises)."""
        ids = np.ascontiguousarray(stream_ids, np.int64).reshape(-1)
        noise = np.zeros((max(ids.size, 1), 1024), np.float32)
        seen = np.zeros(max(ids.size, 1), np.int64)
        self.eng._ck(L.jdsp_denoise_streams_state(self._h, _vp(ids), ids.size, _vp(noise), _vp(seen)))
        return noise[:ids.size], seen[:ids.size]

    # ---- one rank's share of a global stream (jdsp_denoise_shard_*; driver: sharding.denoise_sharded)
    def shard_vad(self, pcm_ext, ext0, b0, b1, n_total):
        import torch
        flags = torch.empty(max(b1 - b0, 1), dtype=torch.uint8, device=pcm_ext.device)
        self.eng._use_torch_stream()
        self.eng._ck(L.jdsp_denoise_shard_vad_dev(self._h, C.c_void_p(pcm_ext.data_ptr()), ext0, b0, b1, n_total,
                                                  C.c_void_p(flags.data_ptr())))
        return flags[: b1 - b0]

    def shard_summary(self, flags_all):
        import torch
        out = torch.empty(1025, dtype=torch.float32, device=flags_all.device)
        self.eng._use_torch_stream()
        self.eng._ck(L.jdsp_denoise_shard_summary_dev(self._h, C.c_void_p(flags_all.data_ptr()), C.c_void_p(out.data_ptr())))
        return out

    def shard_rows(self, summaries_all, world, rank):
        import torch
        out = torch.empty(1025, dtype=torch.float32, device=summaries_all.device)
        self.eng._use_torch_stream()
        self.eng._ck(L.jdsp_denoise_shard_rows_dev(self._h, C.c_void_p(summaries_all.data_ptr()), world, rank,
                                                   C.c_void_p(out.data_ptr())))
        return out

    def shard_finish(self, last_all, world, rank, want_precast=False):
        import torch
        n_out = L.jdsp_denoise_shard_blocks_out(self._h)
        B = self.block
        out = torch.empty(max(n_out, 1) * B, dtype=torch.int16, device=last_all.device)
        pre = torch.empty(max(n_out, 1) * B, dtype=torch.float32, device=last_all.device) if want_precast else None
        self.eng._use_torch_stream()
        self.eng._ck(L.jdsp_denoise_shard_finish_dev(self._h, C.c_void_p(last_all.data_ptr()), world, rank,
                                                     C.c_void_p(out.data_ptr()),
                                                     C.c_void_p(pre.data_ptr()) if want_precast else None, None))
        return (out[: n_out * B], pre[: n_out * B]) if want_precast else out[: n_out * B]

    def apply(self, pcm, noise, want_precast=False):
        """SpectralSubtraction / WienerFiltering (SS:201-264 / WF:162-235) over whole blocks with the CALLER's
        pdEstimatedNoiseSpec (n_fft doubles) instead of the handle's own VAD + estimate (jdsp_denoise_apply; host)."""
        B = self.block
        pcm = np.ascontiguousarray(pcm, np.int16)
        noise = np.ascontiguousarray(noise, np.float64)
        assert pcm.size % B == 0 and noise.size == self.n_fft
        nb = pcm.size // B
        n_out = self.blocks_out(nb)
        out = np.zeros(max(n_out, 1) * B, np.int16)
        pre = np.zeros(max(n_out, 1) * B, np.float32) if want_precast else None
        self.eng._ck(L.jdsp_denoise_apply(self._h, _vp(pcm), nb, _vp(noise), _vp(out), _vp(pre), None))
        return (out[:n_out * B], pre[:n_out * B]) if want_precast else out[:n_out * B]

    def noise(self):
        n = np.zeros(self.n_fft, np.float64)
        self.eng._ck(L.jdsp_denoise_noise(self._h, n.ctypes.data_as(C.c_void_p)))
        return n

    def frames_recomputed(self):
        """Spectral-subtraction frames of the last call that went through the FP64 pass (jdsp_denoise_frames_recomputed)."""
        n = L.jdsp_denoise_frames_recomputed(self._h)
        if n < 0:
            self.eng._ck(int(n))
        return int(n)

    def vad_trace(self, n, flags_only=False):
        """(voice, energy sums, ZCR) of the last call's first n blocks; energies / ZCR need set_option("vad_trace", 1)
        before that call (flags_only=True asks for the flags alone, which are always kept)."""
        if flags_only:
            v = np.zeros(n, np.uint8)
            self.eng._ck(L.jdsp_denoise_vad_trace(self._h, n, v.ctypes.data_as(C.c_void_p), None, None))
            return v
        v = np.zeros(n, np.uint8)
        e = np.zeros(n, np.int64)
        z = np.zeros(n, np.int32)
        self.eng._ck(L.jdsp_denoise_vad_trace(self._h, n, v.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p),
                                              z.ctypes.data_as(C.c_void_p)))
        return v, e, z


class Mfcc(_Child):
    """MFCC front end (jdsp_mfcc): MFCCFeatureExtraction_auto_version1.cpp for batches of frames.
    Keyword arguments override the reference-native configuration (jdsp_mfcc_native_cfg)."""
    _destroy = staticmethod(lambda h: L.jdsp_mfcc_destroy(h))

    def __init__(self, engine, **kw):
        self.eng = engine
        cfg = _lib.MfccCfg()
        engine._ck(L.jdsp_mfcc_native_cfg(C.byref(cfg)))
        for k, v in kw.items():
            setattr(cfg, k, v)
        self.cfg = cfg
        h = C.c_void_p()
        engine._ck(L.jdsp_mfcc_create(engine._h, C.byref(cfg), C.byref(h)))
        self._h = h
        engine._children.append(self)

    def tables(self):
        """MelFilterBankInit's rgdMelFreqs, rgdFiBins, rgdFilterBank."""
        nb = self.cfg.n_fft // 2
        mel = np.zeros(self.cfg.n_chan + 1, np.float64)
        fi = np.zeros(nb, np.int32)
        fb = np.zeros(nb, np.float64)
        self.eng._ck(L.jdsp_mfcc_tables(self._h, mel.ctypes.data_as(C.c_void_p), fi.ctypes.data_as(C.c_void_p),
                                        fb.ctypes.data_as(C.c_void_p)))
        return mel, fi, fb

    def n_frames(self, n_samples):
        return (n_samples - self.cfg.win_len) // self.cfg.hop + 1 if n_samples >= self.cfg.win_len else 0

    # ---- the sub-steps on their own (MFCC:154-192), FP64, rows = independent frames
    def mel_filterbank(self, mag):
        """MelFilterBank: |X| [rows, n_fft/2] -> ln channel sums [rows, n_chan]."""
        mag = np.ascontiguousarray(np.atleast_2d(mag), np.float64)
        assert mag.shape[1] == self.cfg.n_fft // 2
        out = np.empty((mag.shape[0], self.cfg.n_chan), np.float64)
        self.eng._ck(L.jdsp_mfcc_melfilterbank(self._h, _vp(mag), mag.shape[0], _vp(out)))
        return out

    def dct(self, mel, accumulate_into=None):
        """DCT: [rows, n_chan] -> [rows, n_cep], ADDED to accumulate_into (default zeros) like the reference."""
        mel = np.ascontiguousarray(np.atleast_2d(mel), np.float64)
        assert mel.shape[1] == self.cfg.n_chan
        out = np.zeros((mel.shape[0], self.cfg.n_cep), np.float64) if accumulate_into is None else \
            np.ascontiguousarray(np.atleast_2d(accumulate_into), np.float64).copy()
        assert out.shape == (mel.shape[0], self.cfg.n_cep)
        self.eng._ck(L.jdsp_mfcc_dct(self._h, _vp(mel), mel.shape[0], _vp(out)))
        return out

    def liftering(self, cep):
        cep = np.ascontiguousarray(np.atleast_2d(cep), np.float64).copy()
        assert cep.shape[1] == self.cfg.n_cep
        self.eng._ck(L.jdsp_mfcc_liftering(self._h, _vp(cep), cep.shape[0]))
        return cep

    def frames(self, pcm, n_frames=None, frame_start=None, out=None):
        """Feature vectors [n_frames, n_cep] float64; frame j starts at frame_start[j] (default hop*j).
        out (device path only): a caller-owned [n_frames, n_cep] float64 CUDA tensor (no allocation: graph capture)."""
        if _is_torch(pcm):
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
            if n_frames is None:
                n_frames = len(frame_start) if frame_start is not None else self.n_frames(pcm.numel())
            if out is None:
                out = torch.empty((n_frames, self.cfg.n_cep), dtype=torch.float64, device=pcm.device)
            assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= n_frames * self.cfg.n_cep
            if frame_start is not None:
                assert frame_start.is_cuda and frame_start.dtype == torch.int64 and frame_start.numel() >= n_frames
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_mfcc_frames_dev(self._h, C.c_void_p(pcm.data_ptr()),
                                                C.c_void_p(frame_start.data_ptr()) if frame_start is not None else None,
                                                n_frames, C.c_void_p(out.data_ptr())))
            return out
        pcm = np.ascontiguousarray(pcm, np.int16)
        if frame_start is not None:
            frame_start = np.ascontiguousarray(frame_start, np.int64)
        if n_frames is None:
            n_frames = len(frame_start) if frame_start is not None else self.n_frames(pcm.size)
        out = np.zeros((n_frames, self.cfg.n_cep), np.float64)
        self.eng._ck(L.jdsp_mfcc_frames(self._h, pcm.ctypes.data_as(C.c_void_p), pcm.size,
                                        frame_start.ctypes.data_as(C.c_void_p) if frame_start is not None else None,
                                        n_frames, out.ctypes.data_as(C.c_void_p)))
        return out


# numpy views of the reference's parameter records (GMMAlgorithm_Test_Auto_ver2.cpp:29-34,
# Viterbi_version1.cpp:30-40): np.fromfile(path, GMM_PARAM) reads a parameter file
GMM_PARAM = np.dtype([("alpa", "<f8", (4,)), ("mean", "<f8", (4, 12)), ("covariance", "<f8", (4, 12, 12)),
                      ("eigenVector", "<f8", (4, 12, 4))])
HMM_PARAM = np.dtype([("gMMParam", GMM_PARAM, (6,)), ("transProb", "<f8", (6, 6))])
# the training program's record (GMMAlgorithm_Train_Auto_ver2.cpp:26-32, PCA_LEN 8): 8,096 bytes
GMM_TRAIN_PARAM = np.dtype([("alpa", "<f8", (4,)), ("mean", "<f8", (4, 12)), ("covariance", "<f8", (4, 12, 12)),
                            ("eigenVector", "<f8", (4, 12, 8))])
# jdsp_gmm_train_stats
GMM_TRAIN_STATS = np.dtype([("kmeans_passes", "<i4"), ("kmeans_capped", "<i4"), ("selected", "<i4", (4,)),
                            ("files", "<i4"), ("status", "<i4"), ("kmeans_cost", "<f8")])


def to_score_params(records):
    """GMM_TRAIN_PARAM records -> the GMM_PARAM records Engine.gmm() scores with (jdsp_gmm_param_from_train: the first
    four eigenvector columns, as GMMAlgorithm_Test_Auto_ver2.cpp:216-235 reads them; everything else copied).
    Host only."""
    records = np.ascontiguousarray(records, GMM_TRAIN_PARAM).reshape(-1)
    out = np.zeros(len(records), GMM_PARAM)
    rc = L.jdsp_gmm_param_from_train(_vp(records), len(records), _vp(out))
    if rc != 0:
        raise JdspError(rc, "jdsp_gmm_param_from_train")
    return out


def _vp(a):
    if a is None:
        return None
    if _is_torch(a):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


class Gmm(_Child):
    """GMM scoring (jdsp_gmm): Recognition() of GMMAlgorithm_Test_Auto_ver2.cpp for batches of utterances.
    `classes`: numpy array of GMM_PARAM records, one per class."""
    _destroy = staticmethod(lambda h: L.jdsp_gmm_destroy(h))

    def __init__(self, engine, classes):
        self.eng = engine
        classes = np.ascontiguousarray(classes, GMM_PARAM).reshape(-1)
        self.n_classes = len(classes)
        h = C.c_void_p()
        engine._ck(L.jdsp_gmm_create(engine._h, _vp(classes), self.n_classes, C.byref(h)))
        self._h = h
        engine._children.append(self)

    def set_option(self, name, value):
        self.eng._ck(L.jdsp_gmm_set_option(self._h, name.encode(), int(value)))

    def score(self, feats, utt_first):
        """feats [n_vectors, 12] float64, utt_first [n_utts + 1] int64 -> (scores [n_utts, n_classes], best [n_utts]).
        torch CUDA tensors stay on the device; numpy arrays go through the host entry."""
        n_utts = len(utt_first) - 1
        if _is_torch(feats):
            import torch
            assert feats.is_cuda and feats.dtype == torch.float64 and feats.is_contiguous()
            assert utt_first.is_cuda and utt_first.dtype == torch.int64
            scores = torch.empty((n_utts, self.n_classes), dtype=torch.float64, device=feats.device)
            best = torch.empty((n_utts,), dtype=torch.int32, device=feats.device)
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_gmm_score_dev(self._h, _vp(feats), feats.shape[0], _vp(utt_first), n_utts, _vp(scores),
                                              _vp(best)))
            return scores, best
        feats = np.ascontiguousarray(feats, np.float64)
        utt_first = np.ascontiguousarray(utt_first, np.int64)
        scores = np.empty((n_utts, self.n_classes), np.float64)
        best = np.empty((n_utts,), np.int32)
        self.eng._ck(L.jdsp_gmm_score(self._h, _vp(feats), _vp(utt_first), n_utts, _vp(scores), _vp(best)))
        return scores, best


class Hmm(_Child):
    """Six-state HMM recursion (jdsp_hmm): HMMRecognition() of Viterbi_version1.cpp for batches of utterances.
    `models`: numpy array of HMM_PARAM records."""
    _destroy = staticmethod(lambda h: L.jdsp_hmm_destroy(h))

    def __init__(self, engine, models):
        self.eng = engine
        models = np.ascontiguousarray(models, HMM_PARAM).reshape(-1)
        self.n_models = len(models)
        h = C.c_void_p()
        engine._ck(L.jdsp_hmm_create(engine._h, _vp(models), self.n_models, C.byref(h)))
        self._h = h
        engine._children.append(self)

    def set_option(self, name, value):
        self.eng._ck(L.jdsp_hmm_set_option(self._h, name.encode(), int(value)))

    def viterbi(self, feats, utt_first, want_path=True, want_trellis=False):
        """-> (scores [n_utts, n_models], best [n_utts], path [n_models, n_vectors] or None[, trellis])."""
        n_utts = len(utt_first) - 1
        n_frames = feats.shape[0]
        if _is_torch(feats):
            import torch
            assert feats.is_cuda and feats.dtype == torch.float64 and feats.is_contiguous()
            assert utt_first.is_cuda and utt_first.dtype == torch.int64
            dev = feats.device
            scores = torch.empty((n_utts, self.n_models), dtype=torch.float64, device=dev)
            best = torch.empty((n_utts,), dtype=torch.int32, device=dev)
            path = torch.zeros((self.n_models, n_frames), dtype=torch.int32, device=dev) if want_path else None
            trellis = torch.zeros((self.n_models, 6, n_frames), dtype=torch.float64, device=dev) if want_trellis else None
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_hmm_viterbi_dev(self._h, _vp(feats), n_frames, _vp(utt_first), n_utts, _vp(scores),
                                                _vp(best), _vp(path), _vp(trellis)))
            return (scores, best, path, trellis) if want_trellis else (scores, best, path)
        feats = np.ascontiguousarray(feats, np.float64)
        utt_first = np.ascontiguousarray(utt_first, np.int64)
        scores = np.empty((n_utts, self.n_models), np.float64)
        best = np.empty((n_utts,), np.int32)
        path = np.zeros((self.n_models, n_frames), np.int32) if want_path else None
        trellis = np.zeros((self.n_models, 6, n_frames), np.float64) if want_trellis else None
        self.eng._ck(L.jdsp_hmm_viterbi(self._h, _vp(feats), _vp(utt_first), n_utts, _vp(scores), _vp(best), _vp(path),
                                        _vp(trellis)))
        return (scores, best, path, trellis) if want_trellis else (scores, best, path)


class FastConv(_Child):
    """Overlap-save convolver (jdsp_fastconv): AnalySisFreqDomain of
    Fast_Convolution_Based_3DAudio_Impl.cpp:102-177 for batches of blocks.
    taps: [n_taps] or [n_filters, n_taps] float64."""
    _destroy = staticmethod(lambda h: L.jdsp_fastconv_destroy(h))

    def __init__(self, engine, taps, n_fft):
        self.eng = engine
        taps = np.ascontiguousarray(np.atleast_2d(np.asarray(taps, np.float64)))
        self.n_filters, self.n_taps = taps.shape
        h = C.c_void_p()
        engine._ck(L.jdsp_fastconv_create(engine._h, taps.ctypes.data_as(C.c_void_p), self.n_taps, self.n_filters,
                                          int(n_fft), C.byref(h)))
        self._h = h
        self.block = L.jdsp_fastconv_block_len(h)
        self.hist_blocks = L.jdsp_fastconv_hist_blocks(h)
        engine._children.append(self)

    def reset(self):
        self.eng._ck(L.jdsp_fastconv_reset(self._h))

    def set_position(self, blocks_consumed):
        self.eng._ck(L.jdsp_fastconv_set_position(self._h, int(blocks_consumed)))

    def blocks_out(self, n_blocks):
        return L.jdsp_fastconv_blocks_out(self._h, n_blocks)

    def process(self, pcm, want_precast=False):
        """pcm: int16, whole blocks of self.block samples.  Returns out [n_filters, n_out*block] (and precast)."""
        if _is_torch(pcm):
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous() and pcm.numel() % self.block == 0
            nb = pcm.numel() // self.block
            n_out = self.blocks_out(nb)
            shape = (self.n_filters, max(n_out, 1) * self.block)
            out = torch.empty(shape, dtype=torch.int16, device=pcm.device)
            pre = torch.empty(shape, dtype=torch.float32, device=pcm.device) if want_precast else None
            if n_out == 0:
                out, pre = out[:, :0], (pre[:, :0] if want_precast else None)
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_fastconv_process_dev(self._h, C.c_void_p(pcm.data_ptr()), nb, C.c_void_p(out.data_ptr()),
                                                     C.c_void_p(pre.data_ptr()) if want_precast else None, None))
            return (out, pre) if want_precast else out
        pcm = np.ascontiguousarray(pcm, np.int16)
        assert pcm.size % self.block == 0
        nb = pcm.size // self.block
        n_out = self.blocks_out(nb)
        out = np.zeros((self.n_filters, n_out * self.block), np.int16)
        pre = np.zeros((self.n_filters, n_out * self.block), np.float32) if want_precast else None
        dummy = np.zeros(1, np.int16)
        self.eng._ck(L.jdsp_fastconv_process(self._h, pcm.ctypes.data_as(C.c_void_p), nb,
                                             (out if out.size else dummy).ctypes.data_as(C.c_void_p),
                                             pre.ctypes.data_as(C.c_void_p) if (want_precast and pre.size) else None, None))
        return (out, pre) if want_precast else out


class Reverb(_Child):
    """Batched reverberation (jdsp_reverb; NOT a reference function: the partitioned overlap-save convolver of
    FastConv over a batch of ragged utterances, each with its own response out of a bank and its own gain).
    taps: [n_irs, n_taps] (or [n_taps]) float64, n_taps <= 7680.  Blocks are self.block = 512 samples.  The same
    arithmetic over live streams whose history the handle carries: open_streams / process_streams."""
    _destroy = staticmethod(lambda h: L.jdsp_reverb_destroy(h))

    def __init__(self, engine, taps):
        self.eng = engine
        taps = np.ascontiguousarray(np.atleast_2d(np.asarray(taps, np.float64)))
        assert taps.ndim == 2, "taps: [n_irs, n_taps]"
        self.n_irs, self.n_taps = taps.shape
        h = C.c_void_p()
        engine._ck(L.jdsp_reverb_create(engine._h, _vp(taps), self.n_irs, self.n_taps, C.byref(h)))
        self._h = h
        self.block = L.jdsp_reverb_block_len(h)
        self.n_part = L.jdsp_reverb_n_part(h)
        engine._children.append(self)

    def reserve_batch(self, n_blocks, n_utts):
        """Sizes the workspace of process_batch's device path (jdsp_reverb_batch_reserve): the only call of the batch
        entries that allocates.  Call it before capturing process_batch in a graph."""
        self.eng._ck(L.jdsp_reverb_batch_reserve(self._h, int(n_blocks), int(n_utts)))

    def process_batch(self, pcm, sample_first, block_first, ir, gain=None, want_f32=False, out=None, out_f32=None):
        """A batch of independent utterances in one launch sequence (jdsp_reverb_batch): utterance u is the
        block_first[u + 1] - block_first[u] blocks of self.block samples at pcm[sample_first[u]] (the layout of
        Denoiser.process_batch; sharding.denoise_batch_layout packs one), convolved with response ir[u] of the bank at
        gain[u] (None: 1), silence in front of it.  pcm: int16; sample_first [n_utts], block_first [n_utts + 1], ir
        [n_utts] and gain [n_utts]: host sequences.  torch CUDA pcm (the device entry on torch's current stream, the
        four arrays copied over first and the workspace reserved on demand: a graph captures the C entry on arrays of its
        own, after reserve_batch) or numpy (the host entry, which also checks the arrays).  Returns int16 of pcm's length, TIME-ALIGNED with pcm; outside
        the spans it is zero, or left as it was in `out` / `out_f32` when given on the device path.  With want_f32:
        (out, float32 values before the cast)."""
        assert pcm.ndim == 1
        n_samples = int(pcm.shape[0])
        sample_first = np.ascontiguousarray(sample_first, np.int64).reshape(-1)
        block_first = np.ascontiguousarray(block_first, np.int64).reshape(-1)
        ir = np.ascontiguousarray(ir, np.int32).reshape(-1)
        gain = None if gain is None else np.ascontiguousarray(gain, np.float32).reshape(-1)
        n_utts = ir.size
        assert sample_first.size == n_utts and block_first.size == n_utts + 1 and (gain is None or gain.size == n_utts)
        dev = pcm.device if _is_torch(pcm) else None
        o16 = _batch_out(n_samples, np.int16, dev, out)
        o32 = _batch_out(n_samples, np.float32, dev, out_f32) if (want_f32 or out_f32 is not None) else None
        if dev is not None:
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
            n_total = int(block_first[-1])
            d_first, d_block, d_ir = (torch.from_numpy(a).to(dev) for a in (sample_first, block_first, ir))
            d_gain = None if gain is None else torch.from_numpy(gain).to(dev)
            self.reserve_batch(n_total, n_utts)                 # a no-op once sized
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_reverb_batch_dev(self._h, _vp(pcm), _vp(d_first), _vp(d_block), _vp(d_ir), _vp(d_gain),
                                                 n_utts, n_total, _vp(o16), _vp(o32)))
        else:
            pcm = np.ascontiguousarray(pcm, np.int16)
            self.eng._ck(L.jdsp_reverb_batch(self._h, _vp(pcm), n_samples, _vp(sample_first), _vp(block_first), _vp(ir),
                                             _vp(gain), n_utts, _vp(o16), _vp(o32)))
        return (o16[:n_samples], o32[:n_samples]) if want_f32 else o16[:n_samples]

    # ---- live streams: n independent streams in the handle, advanced a chunk each by one call (jdsp_reverb_streams_*)
    def open_streams(self, n_streams, max_blocks_total):
        """Gives the handle n_streams live streams, all fresh, and the workspace of calls of up to max_blocks_total
        blocks (jdsp_reverb_streams_reserve): the only call of the live entries that allocates, and it synchronises.
        1,032 + 4,160 (n_part - 1) bytes of state per stream.  Calling it again discards every live stream's state."""
        self.eng._ck(L.jdsp_reverb_streams_reserve(self._h, int(n_streams), int(max_blocks_total)))
        self.n_streams = int(n_streams)
        self._streams_torch = None      # the kind of the last process_streams() input
        self._streams_key = None

    def process_streams(self, pcm, stream_ids, block_counts, ir, gain=None, chunk_sample_first=None, want_f32=False,
                        out=None, out_f32=None):
        """One call over live streams (jdsp_reverb_streams; open_streams first): chunk c continues the live stream
        stream_ids[c] with block_counts[c] >= 0 NEW blocks of self.block samples at chunk_sample_first[c] of pcm int16
        [n_samples] (even, ascending, disjoint; None: back to back, sharding.denoise_batch_layout), convolved with
        response ir[c] at gain[c] (None: 1) over everything the stream has been given so far.  Ids are distinct within
        a call.  torch CUDA (the device entry on torch's current stream) or numpy (the host entry, which also checks
        the arrays).  Returns int16 [n_samples], TIME-ALIGNED with pcm; outside the spans it is zero, or left as it was
        in `out` / `out_f32` when given on the device path.  A stream's result does not depend, bit for bit, on how its
        blocks are cut into chunks and calls, and with one (ir, gain) throughout it is process_batch's of the whole
        stream as one utterance.  With want_f32: (out, float32 values before the cast)."""
        from .sharding import denoise_batch_layout
        ids = np.ascontiguousarray(stream_ids, np.int64).reshape(-1)
        counts = np.ascontiguousarray(block_counts, np.int64).reshape(-1)
        ir = np.ascontiguousarray(ir, np.int32).reshape(-1)
        gain = None if gain is None else np.ascontiguousarray(gain, np.float32).reshape(-1)
        assert ids.size == counts.size == ir.size and (gain is None or gain.size == ids.size), "one entry per chunk"
        packed, block_first, _ = denoise_batch_layout(counts, self.block)
        if chunk_sample_first is None:
            sample_first = packed
        else:
            sample_first = np.ascontiguousarray(chunk_sample_first, np.int64).reshape(-1)
            assert sample_first.size == ids.size
        assert pcm.ndim == 1
        n_chunks, n_total, n_samples = ids.size, int(block_first[-1]), int(pcm.shape[0])
        dev = pcm.device if _is_torch(pcm) else None
        self._streams_torch = dev
        o16 = _batch_out(n_samples, np.int16, dev, out)
        o32 = _batch_out(n_samples, np.float32, dev, out_f32) if (want_f32 or out_f32 is not None) else None
        if dev is not None:
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
            assert n_chunks == 0 or int((sample_first + counts * self.block).max()) <= n_samples
            key = (ids.tobytes(), sample_first.tobytes(), counts.tobytes(), ir.tobytes(),
                   None if gain is None else gain.tobytes(), dev)
            if self._streams_key != key:
                self._streams_dev = tuple(None if a is None else torch.from_numpy(a).to(dev)
                                          for a in (ids, sample_first, block_first, ir, gain))
                self._streams_key = key
            d_ids, d_sample, d_block, d_ir, d_gain = self._streams_dev
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_reverb_streams_dev(self._h, _vp(pcm), _vp(d_ids), _vp(d_sample), _vp(d_block), _vp(d_ir),
                                                   _vp(d_gain), n_chunks, n_total, _vp(o16), _vp(o32)))
        else:
            pcm = np.ascontiguousarray(pcm, np.int16)
            self.eng._ck(L.jdsp_reverb_streams(self._h, _vp(pcm), n_samples, _vp(ids), _vp(sample_first), _vp(block_first),
                                               _vp(ir), _vp(gain), n_chunks, _vp(o16), _vp(o32)))
        return (o16[:n_samples], o32[:n_samples]) if want_f32 else o16[:n_samples]

    def reset_streams(self, stream_ids=None):
        """The listed live streams fresh again, or all of them with None (jdsp_reverb_streams_reset_dev; enqueue-only)."""
        if stream_ids is None:
            if self._streams_torch is not None:
                self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_reverb_streams_reset_dev(self._h, None, 0))
            return
        import torch
        ids = np.ascontiguousarray(stream_ids, np.int64).reshape(-1)
        dev = self._streams_torch if self._streams_torch is not None else torch.device("cuda", self.eng.device)
        d_ids = torch.from_numpy(ids).to(dev)
        self.eng._use_torch_stream()
        self.eng._ck(L.jdsp_reverb_streams_reset_dev(self._h, _vp(d_ids), ids.size))
        self._reset_args = d_ids                                # alive until the stream has run the call

    def streams_state(self, stream_ids):
        """(blocks seen int64 [n_ids], the last block's samples int16 [n_ids, 512], zeros for a fresh stream) of the
        listed live streams (jdsp_reverb_streams_state; synchronises)."""
        ids = np.ascontiguousarray(stream_ids, np.int64).reshape(-1)
        seen = np.zeros(max(ids.size, 1), np.int64)
        last = np.zeros((max(ids.size, 1), self.block), np.int16)
        self.eng._ck(L.jdsp_reverb_streams_state(self._h, _vp(ids), ids.size, _vp(seen), _vp(last)))
        return seen[:ids.size], last[:ids.size]


class Binaural(_Child):
    """Live binaural rendering (jdsp_binaural; NOT a reference function: the overlap-save convolver of
    Fast_Convolution_Based_3DAudio_Impl.cpp:102-177 generalised to mixes of moving sources).
    hrirs: [n_dirs, 2, n_taps] float64, n_taps <= 513.  Blocks are self.block = 512 samples."""
    _destroy = staticmethod(lambda h: L.jdsp_binaural_destroy(h))

    def __init__(self, engine, hrirs):
        self.eng = engine
        hrirs = np.ascontiguousarray(np.asarray(hrirs, np.float64))
        assert hrirs.ndim == 3 and hrirs.shape[1] == 2, "hrirs: [n_dirs, 2, n_taps]"
        self.n_dirs, _, self.n_taps = hrirs.shape
        h = C.c_void_p()
        engine._ck(L.jdsp_binaural_create(engine._h, _vp(hrirs), self.n_dirs, self.n_taps, C.byref(h)))
        self._h = h
        self.block = L.jdsp_binaural_block_len(h)
        self.n_streams = 0
        self._streams_torch = None
        engine._children.append(self)

    def open_streams(self, n_streams):
        """Gives the handle n_streams live streams, all fresh (jdsp_binaural_streams_reserve): the only call that
        allocates, and it synchronises.  Calling it again discards every stream."""
        self.eng._ck(L.jdsp_binaural_streams_reserve(self._h, int(n_streams)))
        self.n_streams = int(n_streams)
        self._streams_torch = None

    def render(self, pcm, stream_ids, sample_first, dirs, gains, chunk_first, block_first, plane=None, want_i16=True,
               want_f32=False):
        """One delivery (jdsp_binaural_render; open_streams first): mix m renders block_first[m + 1] - block_first[m]
        blocks from the chunks chunk_first[m] .. chunk_first[m + 1] - 1; chunk c continues stream stream_ids[c] with
        the 512 B_m samples at sample_first[c] of pcm, heard from dirs[c] at gains[c] (sharding.binaural_layout packs
        a delivery; input spans may coincide).  plane: samples per ear of the outputs (None: 512 sum B_m).  pcm torch
        CUDA int16 (the device entry on torch's current stream; the arrays go up with the call) or numpy (the host
        entry, which checks everything).  Returns out_i16 [2, plane] and / or out_f32 [2, plane] as asked (both: a
        tuple); what no block wrote is zero."""
        ids = np.ascontiguousarray(stream_ids, np.int64).reshape(-1)
        sf = np.ascontiguousarray(sample_first, np.int64).reshape(-1)
        d = np.ascontiguousarray(dirs, np.int32).reshape(-1)
        g = np.ascontiguousarray(gains, np.float32).reshape(-1)
        cf = np.ascontiguousarray(chunk_first, np.int64).reshape(-1)
        bf = np.ascontiguousarray(block_first, np.int64).reshape(-1)
        assert ids.size == sf.size == d.size == g.size, "one id, offset, direction and gain per chunk"
        assert cf.size == bf.size and cf.size >= 1, "chunk_first and block_first: [n_mixes + 1]"
        n_mixes, n_chunks, n_total = cf.size - 1, ids.size, int(bf[-1])
        if plane is None:
            plane = self.block * n_total
        plane = int(plane)
        assert pcm.ndim == 1
        n_samples = int(pcm.shape[0])
        dev = pcm.device if _is_torch(pcm) else None
        self._streams_torch = dev
        o16 = _batch_out(2 * plane, np.int16, dev) if want_i16 else None
        o32 = _batch_out(2 * plane, np.float32, dev) if want_f32 else None
        if dev is not None:
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
            counts = np.repeat(np.diff(bf), np.diff(cf)) if n_mixes else np.zeros(0, np.int64)
            assert counts.size == n_chunks and (n_chunks == 0 or int((sf + counts * self.block).max()) <= n_samples)
            self._render_args = tuple(torch.from_numpy(a).to(dev) for a in (ids, sf, d, g, cf, bf))   # alive until run
            a = self._render_args
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_binaural_render_dev(self._h, _vp(pcm), _vp(a[0]), _vp(a[1]), _vp(a[2]), _vp(a[3]),
                                                    _vp(a[4]), _vp(a[5]), n_mixes, n_chunks, n_total, _vp(o16), _vp(o32),
                                                    plane))
        else:
            pcm = np.ascontiguousarray(pcm, np.int16)
            self.eng._ck(L.jdsp_binaural_render(self._h, _vp(pcm), n_samples, _vp(ids), _vp(sf), _vp(d), _vp(g), _vp(cf),
                                                _vp(bf), n_mixes, n_chunks, _vp(o16), _vp(o32), plane))
        res = tuple(o[:2 * plane].reshape(2, plane) for o in (o16, o32) if o is not None)
        return res[0] if len(res) == 1 else (res if res else None)

    def reset_streams(self, stream_ids=None):
        """The listed live streams fresh again, or all of them with None (jdsp_binaural_streams_reset_dev; enqueue-only)."""
        if stream_ids is None:
            if self._streams_torch is not None:
                self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_binaural_streams_reset_dev(self._h, None, 0))
            return
        import torch
        ids = np.ascontiguousarray(stream_ids, np.int64).reshape(-1)
        dev = self._streams_torch if self._streams_torch is not None else torch.device("cuda", self.eng.device)
        d_ids = torch.from_numpy(ids).to(dev)
        self.eng._use_torch_stream()
        self.eng._ck(L.jdsp_binaural_streams_reset_dev(self._h, _vp(d_ids), ids.size))
        self._reset_args = d_ids                                # alive until the stream has run the call

    def streams_state(self, stream_ids):
        """(hist int16 [n_ids, 512], dir int32 [n_ids], gain float32 [n_ids], started int32 [n_ids]) of the listed live
        streams: what each carries into its next delivery (jdsp_binaural_streams_state; synchronises)."""
        ids = np.ascontiguousarray(stream_ids, np.int64).reshape(-1)
        n = max(ids.size, 1)
        hist, d, g, st = np.zeros((n, 512), np.int16), np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        self.eng._ck(L.jdsp_binaural_streams_state(self._h, _vp(ids), ids.size, _vp(hist), _vp(d), _vp(g), _vp(st)))
        return hist[:ids.size], d[:ids.size], g[:ids.size], st[:ids.size]


class Mvdr(_Child):
    """Two-microphone MVDR beamformer (jdsp_mvdr): main()'s loop of BeamForming_MVDR_ver1.cpp:169-231
    for batches of 512-sample blocks per channel."""
    _destroy = staticmethod(lambda h: L.jdsp_mvdr_destroy(h))

    def __init__(self, engine, d_time=0.0):
        self.eng = engine
        h = C.c_void_p()
        engine._ck(L.jdsp_mvdr_create(engine._h, float(d_time), C.byref(h)))
        self._h = h
        engine._children.append(self)

    def reset(self):
        self.eng._ck(L.jdsp_mvdr_reset(self._h))

    def blocks_out(self, n_blocks):
        return L.jdsp_mvdr_blocks_out(self._h, n_blocks)

    def corr(self):
        c = np.zeros(4, np.float64)
        self.eng._ck(L.jdsp_mvdr_corr(self._h, c.ctypes.data_as(C.c_void_p)))
        return c

    def estimate_corr(self, left_frames, right_frames, corr):
        """EstimateSpatialCorrMtx (BeamForming_MVDR_ver1.cpp:244-270): frames [n, 1024] per channel, returns
        corr (4 doubles, row-major) + every frame's contribution."""
        lf = np.ascontiguousarray(np.atleast_2d(left_frames), np.int16)
        rf = np.ascontiguousarray(np.atleast_2d(right_frames), np.int16)
        assert lf.shape == rf.shape and lf.shape[1] == 1024
        c = np.ascontiguousarray(corr, np.float64).reshape(4).copy()
        self.eng._ck(L.jdsp_mvdr_estimate_corr(self._h, _vp(lf), _vp(rf), lf.shape[0], _vp(c)))
        return c

    def apply(self, left, right, corr, want_precast=False):
        """ProcessMVDR (:124-205) for whole blocks with the CALLER's matrix (4 doubles, row-major)."""
        left = np.ascontiguousarray(left, np.int16)
        right = np.ascontiguousarray(right, np.int16)
        c = np.ascontiguousarray(corr, np.float64).reshape(4)
        nb = left.size // 512
        n_out = self.blocks_out(nb)
        out = np.zeros(max(n_out, 1) * 512, np.int16)
        pre = np.zeros(max(n_out, 1) * 512, np.float32) if want_precast else None
        self.eng._ck(L.jdsp_mvdr_apply(self._h, _vp(left), _vp(right), nb, _vp(c), _vp(out), _vp(pre), None))
        return (out[:n_out * 512], pre[:n_out * 512]) if want_precast else out[:n_out * 512]

    # ---- one rank's share of a global stream (jdsp_mvdr_shard_*)
    def shard_vad(self, left_ext, right_ext, ext0, b0, b1, n_total):
        import torch
        flags = torch.empty(max(b1 - b0, 1), dtype=torch.uint8, device=left_ext.device)
        self.eng._use_torch_stream()
        self.eng._ck(L.jdsp_mvdr_shard_vad_dev(self._h, C.c_void_p(left_ext.data_ptr()), C.c_void_p(right_ext.data_ptr()),
                                               ext0, b0, b1, n_total, C.c_void_p(flags.data_ptr())))
        return flags[: b1 - b0]

    def shard_summary(self, flags_all):
        import torch
        out = torch.empty(4, dtype=torch.float64, device=flags_all.device)
        self.eng._use_torch_stream()
        self.eng._ck(L.jdsp_mvdr_shard_summary_dev(self._h, C.c_void_p(flags_all.data_ptr()), C.c_void_p(out.data_ptr())))
        return out

    def shard_finish(self, sums_all, world, rank, want_precast=False):
        import torch
        n_out = L.jdsp_mvdr_shard_blocks_out(self._h)
        out = torch.empty(max(n_out, 1) * 512, dtype=torch.int16, device=sums_all.device)
        pre = torch.empty(max(n_out, 1) * 512, dtype=torch.float32, device=sums_all.device) if want_precast else None
        self.eng._use_torch_stream()
        self.eng._ck(L.jdsp_mvdr_shard_finish_dev(self._h, C.c_void_p(sums_all.data_ptr()), world, rank,
                                                  C.c_void_p(out.data_ptr()),
                                                  C.c_void_p(pre.data_ptr()) if want_precast else None, None))
        out = out[: n_out * 512]
        return (out, pre[: n_out * 512]) if want_precast else out

    def process(self, left, right, want_precast=False):
        if _is_torch(left):
            import torch
            assert left.is_cuda and right.is_cuda and left.dtype == right.dtype == torch.int16
            assert left.is_contiguous() and right.is_contiguous() and left.numel() == right.numel() and left.numel() % 512 == 0
            nb = left.numel() // 512
            n_out = self.blocks_out(nb)
            out = torch.empty(max(n_out, 1) * 512, dtype=torch.int16, device=left.device)
            pre = torch.empty(max(n_out, 1) * 512, dtype=torch.float32, device=left.device) if want_precast else None
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_mvdr_process_dev(self._h, C.c_void_p(left.data_ptr()), C.c_void_p(right.data_ptr()), nb,
                                                 C.c_void_p(out.data_ptr()),
                                                 C.c_void_p(pre.data_ptr()) if want_precast else None, None))
            out = out[:n_out * 512]
            return (out, pre[:n_out * 512]) if want_precast else out
        left = np.ascontiguousarray(left, np.int16)
        right = np.ascontiguousarray(right, np.int16)
        assert left.size == right.size and left.size % 512 == 0
        nb = left.size // 512
        n_out = self.blocks_out(nb)
        out = np.zeros(max(n_out, 1) * 512, np.int16)
        pre = np.zeros(max(n_out, 1) * 512, np.float32) if want_precast else None
        self.eng._ck(L.jdsp_mvdr_process(self._h, left.ctypes.data_as(C.c_void_p), right.ctypes.data_as(C.c_void_p), nb,
                                         out.ctypes.data_as(C.c_void_p),
                                         pre.ctypes.data_as(C.c_void_p) if want_precast else None, None))
        return (out[:n_out * 512], pre[:n_out * 512]) if want_precast else out[:n_out * 512]


class MvdrMulti(_Child):
    """MVDR generalised to n_mics <= 8 with a per-bin covariance (jdsp_mvdrn, BASELINE config 5).
    pcm: int16 [n_mics, n_blocks * block] (planar); block = n_fft / 2 (512, or 256 for 512-point frames)."""
    _destroy = staticmethod(lambda h: L.jdsp_mvdrn_destroy(h))

    def __init__(self, engine, n_mics, delays=None, loading=0.0, n_fft=1024):
        self.eng = engine
        self.n_mics = int(n_mics)
        d = None if delays is None else np.ascontiguousarray(delays, np.float64)      # None: delays_s = NULL, no steering
        assert d is None or d.size == n_mics
        h = C.c_void_p()
        engine._ck(L.jdsp_mvdrn_create_cfg(engine._h, self.n_mics, None if d is None else d.ctypes.data_as(C.c_void_p),
                                           float(loading), int(n_fft), C.byref(h)))
        self._h = h
        self.block = L.jdsp_mvdrn_block_len(h)
        engine._children.append(self)

    def reset(self):
        self.eng._ck(L.jdsp_mvdrn_reset(self._h))

    def blocks_out(self, n_blocks):
        return L.jdsp_mvdrn_blocks_out(self._h, n_blocks)

    def process(self, pcm, want_precast=False):
        B = self.block
        if _is_torch(pcm):
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous() and pcm.dim() == 2
            assert pcm.shape[0] == self.n_mics and pcm.shape[1] % B == 0
            nb = pcm.shape[1] // B
            n_out = self.blocks_out(nb)
            out = torch.empty(max(n_out, 1) * B, dtype=torch.int16, device=pcm.device)
            pre = torch.empty(max(n_out, 1) * B, dtype=torch.float32, device=pcm.device) if want_precast else None
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_mvdrn_process_dev(self._h, C.c_void_p(pcm.data_ptr()), pcm.shape[1], nb,
                                                  C.c_void_p(out.data_ptr()),
                                                  C.c_void_p(pre.data_ptr()) if want_precast else None, None))
            out = out[:n_out * B]
            return (out, pre[:n_out * B]) if want_precast else out
        pcm = np.ascontiguousarray(pcm, np.int16)
        assert pcm.ndim == 2 and pcm.shape[0] == self.n_mics and pcm.shape[1] % B == 0
        nb = pcm.shape[1] // B
        n_out = self.blocks_out(nb)
        out = np.zeros(max(n_out, 1) * B, np.int16)
        pre = np.zeros(max(n_out, 1) * B, np.float32) if want_precast else None
        self.eng._ck(L.jdsp_mvdrn_process(self._h, pcm.ctypes.data_as(C.c_void_p), pcm.shape[1], nb,
                                          out.ctypes.data_as(C.c_void_p),
                                          pre.ctypes.data_as(C.c_void_p) if want_precast else None, None))
        return (out[:n_out * B], pre[:n_out * B]) if want_precast else out[:n_out * B]

    def reserve_batch(self, max_blocks_total, max_utts):
        """Sizes the workspace of process_batch's device path (jdsp_mvdrn_batch_reserve): the only call of the batch
        entries that allocates.  Call it before capturing process_batch in a graph."""
        self.eng._ck(L.jdsp_mvdrn_batch_reserve(self._h, int(max_blocks_total), int(max_utts)))

    def process_batch(self, pcm, block_counts, utt_sample_first=None, want_precast=False, want_flags=False, out=None):
        """A batch of independent utterances in one launch sequence (jdsp_mvdrn_batch): each comes out as a fresh
        handle's process of its blocks, and the handle's own stream is neither read nor advanced.  1024-point handles.
        pcm: int16 [n_mics, n_samples]; block_counts: B_u >= 0 blocks of 512 samples per utterance (a host sequence);
        utt_sample_first: the n_utts even sample offsets of the spans, the same on every plane, ascending and disjoint
        (None: packed back to back, sharding.denoise_batch_layout).  torch CUDA (the device entry on torch's current
        stream; rows may be strided by a multiple of 8 samples; it reserves on demand, so call reserve_batch first
        under graph capture) or numpy (the host entry).  Returns int16 [n_samples], TIME-ALIGNED with pcm: the
        beamformed samples of utterance u's blocks 1 .. B_u - 1 lie where those blocks lie in pcm; everything else is
        zero, or is left as it was in `out` when given on the device path.  With want_precast / want_flags a tuple
        follows the same order: float32 samples before the cast, uint8 VAD decisions of microphone 0 [sum B_u] in
        concatenated block order."""
        from .sharding import denoise_batch_layout
        counts = np.ascontiguousarray(block_counts, np.int64).reshape(-1)
        packed, block_first, n_packed = denoise_batch_layout(counts, self.block)
        if utt_sample_first is None:
            sample_first = packed
        else:
            sample_first = np.ascontiguousarray(utt_sample_first, np.int64).reshape(-1)[:counts.size]
            assert sample_first.size == counts.size
        assert pcm.ndim == 2 and pcm.shape[0] == self.n_mics
        n_utts, n_total, n_samples = counts.size, int(block_first[-1]), int(pcm.shape[1])
        dev = pcm.device if _is_torch(pcm) else None
        if dev is not None:
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.stride(1) == 1
            stride = int(pcm.stride(0))
            assert n_utts == 0 or int((sample_first + counts * self.block).max()) <= n_samples
            key = (sample_first.tobytes(), counts.tobytes())
            d_sample, d_block, fresh = _batch_offsets(self, key, sample_first, block_first, dev)
            if fresh:
                self.reserve_batch(n_total, n_utts)             # a no-op once sized
        else:
            pcm = np.ascontiguousarray(pcm, np.int16)
            stride = n_samples
        out = _batch_out(n_samples, np.int16, dev, out)
        pre = _batch_out(n_samples, np.float32, dev) if want_precast else None
        flags = _batch_out(n_total, np.uint8, dev) if want_flags else None
        if dev is not None:
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_mvdrn_batch_dev(self._h, _vp(pcm), stride, _vp(d_sample), _vp(d_block), n_utts, n_total,
                                                _vp(out), _vp(pre), _vp(flags)))
        else:
            self.eng._ck(L.jdsp_mvdrn_batch(self._h, _vp(pcm), stride, n_samples, _vp(sample_first), _vp(block_first),
                                            n_utts, _vp(out), _vp(pre), _vp(flags)))
        res = [out[:n_samples]]
        if want_precast:
            res.append(pre[:n_samples])
        if want_flags:
            res.append(flags[:n_total])
        return res[0] if len(res) == 1 else tuple(res)

    # ---- live streams: n independent streams in the handle, advanced a chunk each by one call (jdsp_mvdrn_streams_*)
    def open_streams(self, n_streams, max_blocks_total):
        """Gives the handle n_streams live streams, all fresh, and the workspace of calls of up to max_blocks_total
        blocks (jdsp_mvdrn_streams_reserve): the only call of the live entries that allocates, and it synchronises.
        533,516 bytes of state per stream.  Calling it again discards every live stream's state."""
        self.eng._ck(L.jdsp_mvdrn_streams_reserve(self._h, int(n_streams), int(max_blocks_total)))
        self.n_streams = int(n_streams)
        self._streams_torch = None      # the kind of the last process_streams() input
        self._streams_key = None

    def process_streams(self, pcm, stream_ids, block_counts, chunk_sample_first=None, want_precast=False,
                        want_flags=False, out=None):
        """One call over live streams (jdsp_mvdrn_streams; open_streams first): chunk c continues the live stream
        stream_ids[c] with block_counts[c] >= 0 NEW blocks of 512 samples per microphone, at chunk_sample_first[c] of
        every plane of pcm int16 [n_mics, n_samples] (even, ascending, disjoint; None: back to back,
        sharding.denoise_batch_layout).  Ids are distinct within a call.  torch CUDA (the device entry on torch's
        current stream; rows may be strided by a multiple of 8 samples) or numpy (the host entry).  Returns int16
        [n_samples], TIME-ALIGNED with pcm: every block is beamformed with the block before it, carried from the
        stream's last call where it is the chunk's first, and lies where it lies in pcm; block 0 of a stream's life
        (sharding.mvdrn_stream_written) and everything outside the spans is zero, or is left as it was in `out` when
        given on the device path.  A stream's result does not depend, bit for bit, on how its blocks are cut into
        chunks and calls.  With want_precast / want_flags a tuple follows the same order: float32 samples before the
        cast, uint8 VAD decisions of microphone 0 [sum B_c] in concatenated block order."""
        from .sharding import denoise_batch_layout
        ids = np.ascontiguousarray(stream_ids, np.int64).reshape(-1)
        counts = np.ascontiguousarray(block_counts, np.int64).reshape(-1)
        assert ids.size == counts.size, "one block count per chunk"
        packed, block_first, _ = denoise_batch_layout(counts, self.block)
        if chunk_sample_first is None:
            sample_first = packed
        else:
            sample_first = np.ascontiguousarray(chunk_sample_first, np.int64).reshape(-1)
            assert sample_first.size == ids.size
        assert pcm.ndim == 2 and pcm.shape[0] == self.n_mics
        n_chunks, n_total, n_samples = ids.size, int(block_first[-1]), int(pcm.shape[1])
        dev = pcm.device if _is_torch(pcm) else None
        self._streams_torch = dev
        if dev is not None:
            import torch
            assert pcm.is_cuda and pcm.dtype == torch.int16 and (pcm.stride(1) == 1 or n_samples == 0)
            stride = int(pcm.stride(0)) if n_total else 0       # without a block nothing is read
            assert n_chunks == 0 or int((sample_first + counts * self.block).max()) <= n_samples
            key = (ids.tobytes(), sample_first.tobytes(), counts.tobytes(), dev)
            if self._streams_key != key:
                self._streams_dev = tuple(torch.from_numpy(a).to(dev) for a in (ids, sample_first, block_first))
                self._streams_key = key
            d_ids, d_sample, d_block = self._streams_dev
        else:
            pcm = np.ascontiguousarray(pcm, np.int16)
            stride = n_samples
        out = _batch_out(n_samples, np.int16, dev, out)
        pre = _batch_out(n_samples, np.float32, dev) if want_precast else None
        flags = _batch_out(n_total, np.uint8, dev) if want_flags else None
        if dev is not None:
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_mvdrn_streams_dev(self._h, _vp(pcm), stride, _vp(d_ids), _vp(d_sample), _vp(d_block),
                                                  n_chunks, n_total, _vp(out), _vp(pre), _vp(flags)))
        else:
            self.eng._ck(L.jdsp_mvdrn_streams(self._h, _vp(pcm), stride, n_samples, _vp(ids), _vp(sample_first),
                                              _vp(block_first), n_chunks, _vp(out), _vp(pre), _vp(flags)))
        res = [out[:n_samples]]
        if want_precast:
            res.append(pre[:n_samples])
        if want_flags:
            res.append(flags[:n_total])
        return res[0] if len(res) == 1 else tuple(res)

    def reset_streams(self, stream_ids=None):
        """The listed live streams fresh again, or all of them with None (jdsp_mvdrn_streams_reset_dev; enqueue-only)."""
        if stream_ids is None:
            if self._streams_torch is not None:
                self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_mvdrn_streams_reset_dev(self._h, None, 0))
            return
        import torch
        ids = np.ascontiguousarray(stream_ids, np.int64).reshape(-1)
        dev = self._streams_torch if self._streams_torch is not None else torch.device("cuda", self.eng.device)
        d_ids = torch.from_numpy(ids).to(dev)
        self.eng._use_torch_stream()
        self.eng._ck(L.jdsp_mvdrn_streams_reset_dev(self._h, _vp(d_ids), ids.size))
        self._reset_args = d_ids                                # alive until the stream has run the call

    def streams_state(self, stream_ids, want_cov=False):
        """blocks seen int64 [n_ids] of the listed live streams and, with want_cov, their carried covariances
        complex128 [n_ids, 513, 8, 8] (row, column; zeros for a fresh stream) (jdsp_mvdrn_streams_state; synchronises)."""
        ids = np.ascontiguousarray(stream_ids, np.int64).reshape(-1)
        seen = np.zeros(max(ids.size, 1), np.int64)
        cov = np.zeros((max(ids.size, 1), 513, 8, 8), np.complex128) if want_cov else None
        self.eng._ck(L.jdsp_mvdrn_streams_state(self._h, _vp(ids), ids.size, _vp(seen), _vp(cov)))
        return (seen[:ids.size], cov[:ids.size]) if want_cov else seen[:ids.size]


class _OlaStream(_Child):
    """What Istft and StftMask share, the overlap-add output stream behind both handles: a subclass names its C entry
    points by `_prefix` and hands its inputs to _process()."""
    WINDOWS = {None: _lib.WIN_NONE, "none": _lib.WIN_NONE, "hamming": _lib.WIN_HAMMING, "hann": _lib.WIN_HANN}
    _prefix = None

    @classmethod
    def _c(cls, name):
        return getattr(L, cls._prefix + name)

    @staticmethod
    def _pick(v, names):
        return names[v] if isinstance(v, str) or v is None else int(v)

    def _create(self, engine, cfg):
        self.eng = engine
        h = C.c_void_p()
        engine._ck(self._c("_create")(engine._h, C.byref(cfg), C.byref(h)))
        self._h = h
        self.n_fft, self.hop = cfg.n_fft, cfg.hop
        self._torch = None              # the kind of the last process() input: flush() answers in the same kind
        self.n_streams, self._streams_torch, self._streams_key = 0, None, None     # live streams: open_streams()
        engine._children.append(self)

    def reset(self):
        self.eng._ck(self._c("_reset")(self._h))

    def set_option(self, name, value):
        self.eng._ck(self._c("_set_option")(self._h, name.encode(), int(value)))

    def samples_out(self, n_frames):
        return self._c("_samples_out")(self._h, int(n_frames))

    def _process(self, dev, inputs, n_frames, want_f32, write, out, out_f32):
        """inputs: the C entry's arguments between the handle and the outputs, on the torch device `dev` (the device
        entry on torch's current stream) or, with dev None, in numpy arrays (the host entry)."""
        n_out = self.samples_out(n_frames)
        self._torch = dev
        if not write:
            out = out_f32 = None
        elif dev is not None:
            import torch
            if out is None:
                out = torch.empty(max(n_out, 1), dtype=torch.int16, device=dev)
            if want_f32 and out_f32 is None:
                out_f32 = torch.empty(max(n_out, 1), dtype=torch.float32, device=dev)
        else:
            out = np.zeros(max(n_out, 1), np.int16) if out is None else out
            if want_f32 and out_f32 is None:
                out_f32 = np.zeros(max(n_out, 1), np.float32)
        if dev is not None:
            self.eng._use_torch_stream()
        entry = self._c("_process_dev" if dev is not None else "_process")
        self.eng._ck(entry(self._h, *inputs, n_frames, _vp(out), _vp(out_f32) if want_f32 else None))
        if not write:
            return None
        return (out[:n_out], out_f32[:n_out]) if want_f32 else out[:n_out]

    def _ragged(self, name, dev, inputs, arrays, counts, n_samples, want_f32, out, out_f32):
        """One call of the ragged entry `name` ("_batch" or "_streams"): the device entry on torch's current stream for
        the torch device `dev` or, with dev None, the host entry.  inputs: the C entry's arguments between the handle
        and the offset arrays; arrays: ([ids,] sample_first, frame_first), on dev or in numpy; counts: the scalars
        between them and the outputs.  Returns the n_samples of out, or of (out, out_f32) with want_f32."""
        out = _batch_out(n_samples, np.int16, dev, out)
        out_f32 = _batch_out(n_samples, np.float32, dev, out_f32) if want_f32 else None
        if dev is not None:
            self.eng._use_torch_stream()
        entry = self._c(name + "_dev" if dev is not None else name)
        self.eng._ck(entry(self._h, *inputs, *[_vp(a) for a in arrays], *counts, _vp(out), _vp(out_f32)))
        return (out[:n_samples], out_f32[:n_samples]) if want_f32 else out[:n_samples]

    def flush(self, want_f32=False):
        """The n_fft - hop samples still in the tail; the handle is reset afterwards."""
        n = self.n_fft - self.hop
        if self._torch is not None:
            import torch
            out = torch.zeros(max(n, 1), dtype=torch.int16, device=self._torch)
            f = torch.zeros(max(n, 1), dtype=torch.float32, device=self._torch) if want_f32 else None
            self.eng._use_torch_stream()
            self.eng._ck(self._c("_flush_dev")(self._h, _vp(out), _vp(f)))
        else:
            out = np.zeros(max(n, 1), np.int16)
            f = np.zeros(max(n, 1), np.float32) if want_f32 else None
            self.eng._ck(self._c("_flush")(self._h, _vp(out), _vp(f)))
        return (out[:n], f[:n]) if want_f32 else out[:n]

    # ---- live streams: n independent output streams in the handle, advanced a chunk each by one call ----------------
    def open_streams(self, n_streams):
        """Gives the handle n_streams live streams, all fresh (jdsp_*_streams_reserve): the only call of the live
        entries that allocates, and it synchronises.  Calling it again discards every live stream's state."""
        self.eng._ck(self._c("_streams_reserve")(self._h, int(n_streams)))
        self.n_streams = int(n_streams)
        self._streams_torch = None      # the kind of the last process_streams() input: flush_streams() answers in it
        self._streams_key = None

    def _stream_device(self):
        import torch
        return self._streams_torch if self._streams_torch is not None else torch.device("cuda", self.eng.device)

    def _chunks(self, stream_ids, frame_counts, chunk_sample_first, with_pcm, dev):
        """The arrays of one process_streams call: (ids, sample_first, frame_first) as numpy int64, their device
        copies on `dev` (None with dev None; kept until the layout changes, as _batch_offsets keeps a batch's) and the
        samples the spans reach."""
        from .sharding import stream_chunks_layout
        ids = np.ascontiguousarray(stream_ids, np.int64).reshape(-1)
        counts = np.ascontiguousarray(frame_counts, np.int64).reshape(-1)
        assert ids.size == counts.size, "one frame count per chunk"
        packed, frame_first, _ = stream_chunks_layout(counts, self.n_fft, self.hop, with_pcm)
        if chunk_sample_first is None:
            sample_first = packed
        else:
            sample_first = np.ascontiguousarray(chunk_sample_first, np.int64).reshape(-1)
            assert sample_first.size == ids.size and not np.any(sample_first & 1)
        n = self.n_fft if with_pcm else self.hop
        ends = sample_first + np.where(counts > 0, self.hop * (counts - 1) + n, 0)
        d = None
        if dev is not None:
            import torch
            key = (ids.tobytes(), sample_first.tobytes(), counts.tobytes(), dev)
            if self._streams_key != key:
                self._streams_dev = tuple(torch.from_numpy(a).to(dev) for a in (ids, sample_first, frame_first))
                self._streams_key = key
            d = self._streams_dev
        return ids, sample_first, frame_first, d, int(ends.max()) if ends.size else 0

    def flush_streams(self, stream_ids, want_f32=False):
        """The n_fft - hop samples still in the tail of each listed live stream, then their reset
        (jdsp_*_streams_flush).  Returns int16 [n_ids, n_fft - hop], or (int16, float32) with want_f32, in the kind
        (torch CUDA or numpy) of the last process_streams input."""
        ids = np.ascontiguousarray(stream_ids, np.int64).reshape(-1)
        n = self.n_fft - self.hop
        sample_first = np.arange(ids.size, dtype=np.int64) * n
        total = int(ids.size) * n
        if self._streams_torch is not None:
            import torch
            dev = self._streams_torch
            out = torch.zeros(max(total, 1), dtype=torch.int16, device=dev)
            f = torch.zeros(max(total, 1), dtype=torch.float32, device=dev) if want_f32 else None
            d_ids, d_first = torch.from_numpy(ids).to(dev), torch.from_numpy(sample_first).to(dev)
            self.eng._use_torch_stream()
            self.eng._ck(self._c("_streams_flush_dev")(self._h, _vp(d_ids), _vp(d_first), ids.size, _vp(out), _vp(f)))
            self._flush_args = (d_ids, d_first)                 # alive until the stream has run the call
        else:
            out = np.zeros(max(total, 1), np.int16)
            f = np.zeros(max(total, 1), np.float32) if want_f32 else None
            self.eng._ck(self._c("_streams_flush")(self._h, _vp(ids), _vp(sample_first), ids.size, total, _vp(out),
                                                  _vp(f)))
        out = out[:total].reshape(ids.size, n)
        return (out, f[:total].reshape(ids.size, n)) if want_f32 else out

    def reset_streams(self, stream_ids=None):
        """The listed live streams fresh again, or all of them with None (jdsp_*_streams_reset_dev; enqueue-only)."""
        if stream_ids is None:
            if self._streams_torch is not None:
                self.eng._use_torch_stream()
            self.eng._ck(self._c("_streams_reset_dev")(self._h, None, 0))
            return
        import torch
        ids = np.ascontiguousarray(stream_ids, np.int64).reshape(-1)
        d_ids = torch.from_numpy(ids).to(self._stream_device())
        self.eng._use_torch_stream()
        self.eng._ck(self._c("_streams_reset_dev")(self._h, _vp(d_ids), ids.size))
        self._reset_args = d_ids                                # alive until the stream has run the call


class Istft(_OlaStream):
    """One STFT synthesis output stream (jdsp_istft, include/jdsp.h): spectra -> inverse transform -> synthesis window
    -> overlap-add -> int16 (and optionally the float32 values before the cast).  torch CUDA spectra go through the
    device entry on torch's current stream, numpy spectra through the host entry."""
    _destroy = staticmethod(lambda h: L.jdsp_istft_destroy(h))
    _prefix = "jdsp_istft"
    LAYOUTS = {"full": _lib.SPEC_FULL, "half": _lib.SPEC_HALF}

    def __init__(self, engine, n_fft=1024, hop=512, layout="full", synthesis_window="none", analysis_window="none"):
        pick = self._pick
        self._create(engine, _lib.IstftCfg(int(n_fft), int(hop), pick(layout, self.LAYOUTS),
                                           pick(synthesis_window, self.WINDOWS), pick(analysis_window, self.WINDOWS)))
        self.layout = pick(layout, self.LAYOUTS)
        self.bins = self.n_fft // 2 + 1 if self.layout == _lib.SPEC_HALF else self.n_fft

    @staticmethod
    def _spec(spec):
        """(spec, dev): a torch CUDA complex64 tensor, checked, and its device, or a numpy complex64 array and None"""
        if _is_torch(spec):
            import torch
            assert spec.is_cuda and spec.dtype == torch.complex64 and spec.is_contiguous()
            return spec, spec.device
        return np.ascontiguousarray(spec, np.complex64), None

    def process(self, spec, want_f32=False, out=None, out_f32=None, n_frames=None, write=True):
        """spec: complex64 [n_frames, row_pitch >= bins] (torch CUDA or numpy, rows contiguous).  Returns the int16
        samples of these frames (n_frames * hop), or (int16, float32) with want_f32.  write=False advances the stream
        without writing (both outputs NULL) and returns None."""
        if n_frames is None:
            n_frames = spec.shape[0]
        pitch = spec.shape[-1] if spec.ndim == 2 else self.bins
        spec, dev = self._spec(spec)
        return self._process(dev, (_vp(spec), pitch), n_frames, want_f32, write, out, out_f32)

    def process_batch(self, spec, frame_counts, utt_sample_first=None, want_f32=False, out=None, out_f32=None):
        """A batch of independent utterances in one launch (jdsp_istft_batch): each comes out as a fresh stream's
        process + flush of its rows, bit for bit, and the handle's own stream is neither read nor advanced.
        spec: complex64 [sum F_u, row_pitch >= bins] with contiguous rows, the rows of all utterances back to back
        (Engine.stft_half_batch's output for the half layout); frame_counts: F_u >= 0 per utterance (a host sequence).
        utt_sample_first: the n_utts + 1 even sample offsets of the output spans (utterance u's hop (F_u - 1) + n_fft
        samples start at utt_sample_first[u] and must end at or before utt_sample_first[u + 1]); None packs the spans
        back to back (sharding.istft_batch_layout).  torch CUDA (the device entry on torch's current stream) or numpy
        (the host entry).  Returns int16 of utt_sample_first[-1] samples, or (int16, float32) with want_f32; what lies
        outside the spans is zero, or is left as it was in out / out_f32 when given on the device path."""
        from .sharding import istft_batch_layout
        counts = np.ascontiguousarray(frame_counts, np.int64).reshape(-1)
        packed, frame_first = istft_batch_layout(counts, self.n_fft, self.hop)
        offs = packed if utt_sample_first is None else np.ascontiguousarray(utt_sample_first, np.int64).reshape(-1)
        assert offs.size == counts.size + 1 and not np.any(offs & 1)
        assert np.all(offs[:-1] + (packed[1:] - packed[:-1]) <= offs[1:]), "an utterance's span ends past the next offset"
        n_utts, n_total, n_samples = counts.size, int(frame_first[-1]), int(offs[-1])
        pitch = spec.shape[-1] if spec.ndim == 2 else self.bins
        assert spec.ndim == 2 and spec.shape[0] >= n_total and pitch >= self.bins
        sample_first = np.ascontiguousarray(offs[:-1])
        spec, dev = self._spec(spec)
        if dev is not None:
            key = (offs.tobytes(), counts.tobytes())
            arrays, sizes = _batch_offsets(self, key, sample_first, frame_first, dev)[:2], (n_utts, n_total)
        else:
            arrays, sizes = (sample_first, frame_first), (n_utts, n_samples)
        return self._ragged("_batch", dev, (_vp(spec), pitch), arrays, sizes, n_samples, want_f32, out, out_f32)

    def process_streams(self, spec, stream_ids, frame_counts, chunk_sample_first=None, n_samples=None, want_f32=False,
                        out=None, out_f32=None):
        """One call over live streams (jdsp_istft_streams; open_streams first): chunk c advances the live stream
        stream_ids[c] by the frame_counts[c] >= 0 rows that follow the chunk before it in spec (complex64
        [sum F_c, row_pitch >= bins], contiguous rows) and writes its hop F_c samples at chunk_sample_first[c] (even;
        None packs the chunks back to back, sharding.stream_chunks_layout).  A stream's chunks over the calls followed
        by flush_streams equal a fresh handle's process + flush of the same rows, bit for bit.  Ids are distinct
        within a call.  torch CUDA (the device entry on torch's current stream) or numpy (the host entry).  Returns
        int16 of n_samples (default: up to the last span's end), or (int16, float32) with want_f32; what lies outside
        the written ranges is zero, or is left as it was in out / out_f32 when given on the device path."""
        dev = spec.device if _is_torch(spec) else None
        ids, sample_first, frame_first, d, end = self._chunks(stream_ids, frame_counts, chunk_sample_first, False, dev)
        n_chunks, n_total = ids.size, int(frame_first[-1])
        n_samples = end if n_samples is None else int(n_samples)
        pitch = spec.shape[-1] if spec.ndim == 2 else self.bins
        assert spec.ndim == 2 and spec.shape[0] >= n_total and pitch >= self.bins and n_samples >= end
        self._streams_torch = dev
        spec = self._spec(spec)[0]
        if dev is not None:
            arrays, sizes = d, (n_chunks, n_total)
        else:
            arrays, sizes = (ids, sample_first, frame_first), (n_chunks, n_samples)
        return self._ragged("_streams", dev, (_vp(spec), pitch), arrays, sizes, n_samples, want_f32, out, out_f32)


class StftMask(_OlaStream):
    """One fused STFT masking stream (jdsp_stftmask, include/jdsp.h): int16 PCM -> analysis window -> forward
    transform -> per-bin mask -> inverse transform -> synthesis window -> overlap-add -> int16 (and optionally the
    float32 values before the cast), without the spectrum reaching memory.  torch CUDA inputs go through the device
    entry on torch's current stream, numpy inputs through the host entry."""
    _destroy = staticmethod(lambda h: L.jdsp_stftmask_destroy(h))
    _prefix = "jdsp_stftmask"
    KINDS = {"real": _lib.MASK_REAL, "complex": _lib.MASK_COMPLEX}

    def __init__(self, engine, n_fft=1024, hop=512, analysis_window="hamming", synthesis_window="none", normalise=0,
                 mask_kind="real"):
        pick = self._pick
        self.mask_kind = pick(mask_kind, self.KINDS)
        self._create(engine, _lib.StftMaskCfg(int(n_fft), int(hop), pick(analysis_window, self.WINDOWS),
                                              pick(synthesis_window, self.WINDOWS), int(normalise), self.mask_kind))
        self.bins = self.n_fft // 2 + 1

    def _inputs(self, pcm, mask, n_rows, n_least):
        """(pcm, mask, mask_pitch, dev) of a call over n_rows frames that reads n_least samples: both torch CUDA, checked,
        and their device, or numpy arrays of the handle's types and None"""
        assert pcm.ndim == 1 and pcm.shape[0] >= n_least
        assert mask.ndim in (1, 2) and mask.shape[-1] >= self.bins and (mask.ndim == 1 or mask.shape[0] >= n_rows)
        pitch = mask.shape[1] if mask.ndim == 2 else 0
        if _is_torch(pcm):
            import torch
            want = torch.complex64 if self.mask_kind == _lib.MASK_COMPLEX else torch.float32
            assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()
            assert mask.is_cuda and mask.dtype == want and mask.is_contiguous()
            return pcm, mask, pitch, pcm.device
        pcm = np.ascontiguousarray(pcm, np.int16)
        mask = np.ascontiguousarray(mask, np.complex64 if self.mask_kind == _lib.MASK_COMPLEX else np.float32)
        return pcm, mask, pitch, None

    def process(self, pcm, mask, n_frames=None, want_f32=False, write=True, out=None, out_f32=None):
        """pcm: int16, hop (n_frames - 1) + n_fft samples (n_frames defaults to all the whole frames pcm holds).
        mask: float32 (real) or complex64 (complex); [n_frames, pitch >= bins] with contiguous rows, or 1-D [bins]: one
        row for every frame (pitch 0).  Both torch CUDA or both numpy.  Returns the int16 samples of these frames
        (n_frames * hop), or (int16, float32) with want_f32 (into out / out_f32 when given).  write=False advances the
        stream without writing (both outputs NULL) and returns None."""
        if n_frames is None:
            n_frames = max((pcm.shape[0] - self.n_fft) // self.hop + 1, 0)
        n_frames = int(n_frames)
        n_least = self.hop * (n_frames - 1) + self.n_fft if n_frames else 0
        pcm, mask, pitch, dev = self._inputs(pcm, mask, n_frames, n_least)
        return self._process(dev, (_vp(pcm), _vp(mask), pitch), n_frames, want_f32, write, out, out_f32)

    def frames_recomputed(self):
        """Frames of the last process / process_batch call that went through the FP64 pass
        (jdsp_stftmask_frames_recomputed); waits for the stream."""
        n = L.jdsp_stftmask_frames_recomputed(self._h)
        if n < 0:
            self.eng._ck(int(n))
        return int(n)

    def process_batch(self, pcm, mask, utt_sample_first, want_f32=False, out=None, out_f32=None):
        """A batch of independent utterances in one launch (jdsp_stftmask_batch): each comes out as a fresh stream's
        process + flush of its frames, bit for bit, and the handle's own stream is neither read nor advanced.
        pcm: int16 with the utterances packed at the n_utts + 1 even sample offsets utt_sample_first (a host sequence;
        sharding.stftmask_batch_layout gives each utterance's frame count F_u and first mask row).  mask: float32 or
        complex64 [sum F_u, pitch >= bins] with contiguous rows, or 1-D [bins]: one row for every frame.  Both torch
        CUDA (the device entry on torch's current stream) or both numpy (the host entry).  Returns int16 of pcm's
        length, or (int16, float32) with want_f32: utterance u's hop (F_u - 1) + n_fft samples start at
        utt_sample_first[u]; what lies outside the spans is zero, or is left as it was in out / out_f32 when given on
        the device path."""
        from .sharding import stftmask_batch_layout
        offs = np.ascontiguousarray(utt_sample_first, np.int64).reshape(-1)
        counts, frame_first = stftmask_batch_layout(offs, self.n_fft, self.hop)
        n_utts, n_total, n_samples = counts.size, int(frame_first[-1]), int(pcm.shape[0])
        pcm, mask, pitch, dev = self._inputs(pcm, mask, n_total, int(offs[-1]))
        sample_first = np.ascontiguousarray(offs[:-1])
        if dev is not None:
            inputs, sizes = (_vp(pcm), _vp(mask), pitch), (n_utts, n_total)
            arrays = _batch_offsets(self, offs.tobytes(), sample_first, frame_first, dev)[:2]
        else:
            inputs, sizes = (_vp(pcm), n_samples, _vp(mask), pitch), (n_utts,)
            arrays = (sample_first, frame_first)
        return self._ragged("_batch", dev, inputs, arrays, sizes, n_samples, want_f32, out, out_f32)

    def process_streams(self, pcm, mask, stream_ids, frame_counts, chunk_sample_first=None, want_f32=False, out=None,
                        out_f32=None):
        """One call over live streams (jdsp_stftmask_streams; open_streams first): chunk c advances the live stream
        stream_ids[c] by frame_counts[c] >= 0 frames.  Its PCM span, hop (F_c - 1) + n_fft samples of pcm from
        chunk_sample_first[c] (even; None: the chunks back to back, sharding.stream_chunks_layout), begins with the
        last n_fft - hop samples of the stream's previous chunk -- the handle keeps no PCM -- and its hop F_c output
        samples come out at the same offset; its mask rows follow the chunk before it in mask (float32 or complex64
        [sum F_c, pitch >= bins] with contiguous rows, or 1-D [bins]: one row for everything).  A stream's chunks over
        the calls followed by flush_streams equal a fresh handle's process + flush of the same frames, bit for bit.
        Ids are distinct within a call.  Both torch CUDA (the device entry on torch's current stream) or both numpy
        (the host entry).  Returns int16 of pcm's length, or (int16, float32) with want_f32; what lies outside the
        written ranges is zero, or is left as it was in out / out_f32 when given on the device path."""
        dev = pcm.device if _is_torch(pcm) else None
        ids, sample_first, frame_first, d, end = self._chunks(stream_ids, frame_counts, chunk_sample_first, True, dev)
        n_chunks, n_total, n_samples = ids.size, int(frame_first[-1]), int(pcm.shape[0])
        pcm, mask, pitch = self._inputs(pcm, mask, n_total, end)[:3]
        self._streams_torch = dev
        if dev is not None:
            inputs, arrays, sizes = (_vp(pcm), _vp(mask), pitch), d, (n_chunks, n_total)
        else:
            inputs, sizes = (_vp(pcm), n_samples, _vp(mask), pitch), (n_chunks,)
            arrays = (ids, sample_first, frame_first)
        return self._ragged("_streams", dev, inputs, arrays, sizes, n_samples, want_f32, out, out_f32)


class GmmTrainer(_Child):
    """GMM training (jdsp_gmm_trainer): GMMAlgorithm_Train_Auto_ver2.cpp's per-class file loop on the device.
    The state carries across train() calls; params() reads a PCA-diagonalised copy of it."""
    _destroy = staticmethod(lambda h: L.jdsp_gmm_train_destroy(h))

    def __init__(self, engine, n_classes):
        self.eng = engine
        self.n_classes = int(n_classes)
        h = C.c_void_p()
        engine._ck(L.jdsp_gmm_train_create(engine._h, self.n_classes, C.byref(h)))
        self._h = h
        engine._children.append(self)

    def set_option(self, name, value):
        self.eng._ck(L.jdsp_gmm_train_set_option(self._h, name.encode(), int(value)))

    def reset(self):
        self.eng._ck(L.jdsp_gmm_train_reset(self._h))

    def reserve(self, max_frames, max_files=0):
        self.eng._ck(L.jdsp_gmm_train_reserve(self._h, int(max_frames), int(max_files)))

    def train(self, feats, file_first, file_class):
        """feats [n_vectors, 12] float64; file f = vectors file_first[f] .. file_first[f+1]-1 (int64, n_files + 1),
        of class file_class[f] (int32).  torch CUDA tensors go through the _dev entry on torch's current stream;
        numpy arrays through the validating host entry."""
        n_files = len(file_class)
        if _is_torch(feats):
            import torch
            assert feats.is_cuda and feats.dtype == torch.float64 and feats.is_contiguous()
            assert feats.dim() == 2 and feats.shape[1] == 12
            assert file_first.is_cuda and file_first.dtype == torch.int64 and file_first.is_contiguous()
            assert file_class.is_cuda and file_class.dtype == torch.int32 and file_class.is_contiguous()
            assert file_first.numel() == n_files + 1
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_gmm_train_files_dev(self._h, _vp(feats), feats.shape[0], _vp(file_first),
                                                    _vp(file_class), n_files))
            return
        feats = np.ascontiguousarray(feats, np.float64).reshape(-1, 12)
        file_first = np.ascontiguousarray(file_first, np.int64)
        file_class = np.ascontiguousarray(file_class, np.int32)
        assert file_first.ndim == 1 and file_first.size == n_files + 1
        assert n_files == 0 or len(feats) >= file_first[-1]
        self.eng._ck(L.jdsp_gmm_train_files(self._h, _vp(feats), _vp(file_first), _vp(file_class), n_files))

    def params(self, out=None):
        """-> GMM_TRAIN_PARAM [n_classes] (host).  With `out` a torch CUDA uint8 tensor of n_classes * 8,096 bytes, the
        records are written there by the _dev entry instead (nothing is synchronised)."""
        if out is not None:
            assert _is_torch(out) and out.is_cuda and out.is_contiguous()
            assert out.numel() * out.element_size() >= self.n_classes * GMM_TRAIN_PARAM.itemsize
            assert out.data_ptr() % 8 == 0
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_gmm_train_params_dev(self._h, _vp(out)))
            return out
        rec = np.zeros(self.n_classes, GMM_TRAIN_PARAM)
        self.eng._ck(L.jdsp_gmm_train_params(self._h, _vp(rec), None))
        return rec

    def stats(self):
        """-> GMM_TRAIN_STATS [n_classes]"""
        st = np.zeros(self.n_classes, GMM_TRAIN_STATS)
        self.eng._ck(L.jdsp_gmm_train_params(self._h, None, _vp(st)))
        return st


def geq_design(gain_db=None):
    """CalcCoefficient of 7Band_GEQ.cpp:136-257 on the host (no GPU): float64 [7, 2, 3] = {{b0, b1, b2}, {0, a1, a2}}
    per band; gain_db None = the reference's gains."""
    g = None if gain_db is None else np.ascontiguousarray(gain_db, np.float64)
    assert g is None or g.shape == (7,)
    out = np.zeros((7, 2, 3), np.float64)
    rc = L.jdsp_geq_design(_vp(g) if g is not None else None, _vp(out))
    if rc != 0:
        raise JdspError(rc, "jdsp_geq_design: seven finite gains")
    return out


def _pitch_of(n):
    return max(8, (int(n) + 7) // 8 * 8)


def _streams_host(x, n_streams):
    """int16 [n_streams, n] -> (contiguous [n_streams, pitch] copy, n, pitch), pitch a multiple of 8"""
    x = np.asarray(x, np.int16)
    x = x.reshape(n_streams, -1)
    n = x.shape[1]
    buf = np.zeros((n_streams, _pitch_of(n)), np.int16)
    buf[:, :n] = x
    return buf, n, buf.shape[1]


def _streams_dev(x, n_streams, pitch=None):
    """torch int16 CUDA [n_streams, n] -> (view [n_streams, n] whose row stride is a multiple of 8 and whose base is
    16-byte aligned, n, pitch); copied into a padded tensor only when the caller's layout is not that already"""
    import torch
    assert x.is_cuda and x.dtype == torch.int16
    x = x.reshape(n_streams, -1) if x.dim() != 2 else x
    assert x.shape[0] == n_streams
    n = x.shape[1]
    st = x.stride(0) if n_streams > 1 else (pitch or _pitch_of(n))
    ok = (n == 0 or x.stride(1) == 1) and st % 8 == 0 and st >= n and x.data_ptr() % 16 == 0
    if ok and (pitch is None or st == pitch):
        return x, n, st
    pitch = pitch or _pitch_of(n)
    buf = torch.zeros((n_streams, pitch), dtype=torch.int16, device=x.device)
    buf[:, :n] = x
    return buf[:, :n], n, pitch


class Geq(_Child):
    """Cascade of biquads over n_streams independent int16 streams (jdsp_geq): ApplyIirGEQ of 7Band_GEQ.cpp:259-332,
    every section's output cast to int16.  The state is carried between calls; a stream may be cut anywhere."""
    _destroy = staticmethod(lambda h: L.jdsp_geq_destroy(h))

    def __init__(self, engine, n_streams, coeff=None):
        self.eng = engine
        self.n_streams = int(n_streams)
        if coeff is None:
            self.n_sections, c = 7, None
        else:
            c = np.ascontiguousarray(coeff, np.float64)
            assert c.ndim == 3 and c.shape[1:] == (2, 3)
            self.n_sections = c.shape[0]
        h = C.c_void_p()
        engine._ck(L.jdsp_geq_create(engine._h, _vp(c) if c is not None else None, self.n_sections, self.n_streams,
                                     C.byref(h)))
        self._h = h
        engine._children.append(self)

    def reset(self):
        self.eng._ck(L.jdsp_geq_reset(self._h))

    def state(self):
        """int16 [n_streams, n_sections + 1, 2]: row 0 the last two inputs, row k + 1 the last two outputs of section k"""
        st = np.zeros((self.n_streams, self.n_sections + 1, 2), np.int16)
        self.eng._ck(L.jdsp_geq_get_state(self._h, _vp(st)))
        return st

    def set_state(self, state):
        st = np.ascontiguousarray(state, np.int16)
        assert st.shape == (self.n_streams, self.n_sections + 1, 2)
        self.eng._ck(L.jdsp_geq_set_state(self._h, _vp(st)))

    def process(self, pcm, want_precast=False, out=None):
        """pcm: int16 [n_streams, n] (any n).  Returns out int16 [n_streams, n] (and precast float64 [n_streams, n]).
        out (device tensors only): an int16 [n_streams, pitch] tensor to write into, pitch = pcm's row stride."""
        if _is_torch(pcm):
            import torch
            x, n, pitch = _streams_dev(pcm, self.n_streams)
            if out is None:
                out = torch.zeros((self.n_streams, pitch), dtype=torch.int16, device=x.device)
            assert out.dtype == torch.int16 and out.shape == (self.n_streams, pitch) and out.is_contiguous()
            pre = torch.zeros((self.n_streams, pitch), dtype=torch.float64, device=x.device) if want_precast else None
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_geq_process_dev(self._h, C.c_void_p(x.data_ptr()), n, pitch, C.c_void_p(out.data_ptr()),
                                                C.c_void_p(pre.data_ptr()) if want_precast else None))
            return (out[:, :n], pre[:, :n]) if want_precast else out[:, :n]
        x, n, pitch = _streams_host(pcm, self.n_streams)
        out = np.zeros((self.n_streams, pitch), np.int16)
        pre = np.zeros((self.n_streams, pitch), np.float64) if want_precast else None
        self.eng._ck(L.jdsp_geq_process(self._h, _vp(x), n, pitch, _vp(out), _vp(pre) if want_precast else None))
        return (out[:, :n], pre[:, :n]) if want_precast else out[:, :n]


class Nlms(_Child):
    """Normalised LMS filter over n_streams independent (input, reference) stream pairs (jdsp_nlms): LMSFilter of
    NormalLMS.cpp:96-136 per sample.  Coefficients and the last filter_len - 1 inputs are carried between calls."""
    _destroy = staticmethod(lambda h: L.jdsp_nlms_destroy(h))

    def __init__(self, engine, n_streams, filter_len=256, mu=1e-4, compensation=1e-4):
        self.eng = engine
        self.n_streams, self.filter_len = int(n_streams), int(filter_len)
        h = C.c_void_p()
        engine._ck(L.jdsp_nlms_create(engine._h, self.filter_len, float(mu), float(compensation), self.n_streams,
                                      C.byref(h)))
        self._h = h
        engine._children.append(self)

    def reset(self):
        self.eng._ck(L.jdsp_nlms_reset(self._h))

    def state(self):
        """(coefficients float64 [n_streams, L], keep int16 [n_streams, L - 1], oldest first)"""
        cf = np.zeros((self.n_streams, self.filter_len), np.float64)
        kp = np.zeros((self.n_streams, self.filter_len - 1), np.int16)
        self.eng._ck(L.jdsp_nlms_get_state(self._h, _vp(cf), _vp(kp)))
        return cf, kp

    def set_state(self, coefficients, keep):
        cf = np.ascontiguousarray(coefficients, np.float64)
        kp = np.ascontiguousarray(keep, np.int16)
        assert cf.shape == (self.n_streams, self.filter_len) and kp.shape == (self.n_streams, self.filter_len - 1)
        self.eng._ck(L.jdsp_nlms_set_state(self._h, _vp(cf), _vp(kp)))

    def process(self, x, ref, want_precast=False, out=None):
        """x, ref: int16 [n_streams, n] (any n).  Returns (est, err) int16 [n_streams, n] (and precast float64).
        out (device tensors only): (est, err), int16 [n_streams, pitch] tensors to write into, pitch = x's row stride."""
        if _is_torch(x):
            import torch
            assert _is_torch(ref)
            xv, n, pitch = _streams_dev(x, self.n_streams)
            rv, rn, _ = _streams_dev(ref, self.n_streams, pitch)
            assert rn == n
            if out is None:
                out = tuple(torch.zeros((self.n_streams, pitch), dtype=torch.int16, device=xv.device) for _ in range(2))
            est, err = out
            for t in out:
                assert t.dtype == torch.int16 and t.shape == (self.n_streams, pitch) and t.is_contiguous()
            pre = torch.zeros((self.n_streams, pitch), dtype=torch.float64, device=xv.device) if want_precast else None
            self.eng._use_torch_stream()
            self.eng._ck(L.jdsp_nlms_process_dev(self._h, C.c_void_p(xv.data_ptr()), C.c_void_p(rv.data_ptr()), n, pitch,
                                                 C.c_void_p(est.data_ptr()), C.c_void_p(err.data_ptr()),
                                                 C.c_void_p(pre.data_ptr()) if want_precast else None))
            return (est[:, :n], err[:, :n], pre[:, :n]) if want_precast else (est[:, :n], err[:, :n])
        xv, n, pitch = _streams_host(x, self.n_streams)
        rv, rn, _ = _streams_host(ref, self.n_streams)
        assert rn == n
        est = np.zeros((self.n_streams, pitch), np.int16)
        err = np.zeros((self.n_streams, pitch), np.int16)
        pre = np.zeros((self.n_streams, pitch), np.float64) if want_precast else None
        self.eng._ck(L.jdsp_nlms_process(self._h, _vp(xv), _vp(rv), n, pitch, _vp(est), _vp(err),
                                         _vp(pre) if want_precast else None))
        return (est[:, :n], err[:, :n], pre[:, :n]) if want_precast else (est[:, :n], err[:, :n])
