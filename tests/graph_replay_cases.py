"""What tests/test_graph_replay_gpu.py shares: the one capture helper, byte buffers that live across a capture, and the
case tables of the three classes of "_dev" entries (include/jdsp.h, "Graph capture"):

  S  stateless entries        a replay recomputes from what the buffers hold now
  D  device-resident state    every replay continues the streams
  H  host-carried state       a captured call belongs to the handle's position at capture: one replay, there

Everything inside a capture is a C entry called through ctypes on buffers allocated before it; the graph is one linear
chain on one stream.  Nothing here needs a GPU to import: torch and the library are loaded inside the functions."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FILL = 0xA5                      # every byte of an output buffer before a call: the sentinel of every type
N_UTTS, N_FRAMES = 4, 11         # the ragged batches: four utterances, eleven frames in all


def lib():
    from jeicyboodsp_amd.engine import L
    return L


def sentinel(dtype):
    """the value of `dtype` whose bytes are all FILL"""
    return np.frombuffer(bytes([FILL]) * np.dtype(dtype).itemsize, dtype)[0]


def vp(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def ok(eng, rc, what):
    """a non-zero return code fails the test with jdsp_last_error's text -- inside a capture too"""
    if rc != 0:
        raise AssertionError("%s returned %d: %s" % (what, rc, lib().jdsp_last_error(eng._h).decode()))


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def dev_of(a):
    """a new device buffer (uint8) holding the array's bytes"""
    import torch
    return torch.from_numpy(as_bytes(a).copy()).cuda()


def dev_fill(nbytes):
    import torch
    return torch.full((max(int(nbytes), 1),), FILL, dtype=torch.uint8, device="cuda")


def upload(t, a):
    """new content into a captured buffer: copy_, on the current stream"""
    import torch
    b = as_bytes(a)
    assert b.size == t.numel(), (b.size, t.numel())
    t.copy_(torch.from_numpy(b.copy()))


def download(t, dtype, shape=None):
    a = t.cpu().numpy().view(dtype)
    return a.copy() if shape is None else a.reshape(shape).copy()


def nbytes_of(dtype, shape):
    return int(np.prod(shape)) * np.dtype(dtype).itemsize


def capture(eng, body):
    """The shape bench.py captures with: a side stream that waits for the current one, the capture on it, the current
    stream waiting for it afterwards.  The engine is put on the side stream BEFORE the capture begins, so
    jdsp_set_stream's ordering event is recorded eagerly.  body() calls C entries only and checks their codes."""
    import torch
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        eng._use_torch_stream()
        with torch.cuda.graph(g, stream=side):
            body()
    torch.cuda.current_stream().wait_stream(side)
    return g


def replay(eng, g):
    import torch
    g.replay()
    torch.cuda.synchronize()


def noise_i16(seed, n, sigma=3000.0):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.normal(0, sigma, n)), -32768, 32767).astype(np.int16)


def dealt(R):
    """Three ways to deal N_FRAMES frames among N_UTTS utterances: an empty one (in another place every time), one
    of a single frame, one of R + 2 and the rest."""
    rest = N_FRAMES - 1 - (R + 2)
    assert rest > 0
    return [[0, 1, R + 2, rest], [R + 2, 0, rest, 1], [rest, 1, 0, R + 2]]


# ---- class S: stateless entries ------------------------------------------------------------------------------------
class Stateless:
    """One captured call.  contents: three dicts name -> numpy array (inputs and device-side offset arrays, the same
    sizes every time); outs: name -> (dtype, shape); call(eng, h, B) -> return code, B: name -> device buffer;
    make(eng): a fresh handle or None; reserve(eng, h); outside(content) -> name -> bool mask of the output elements
    that no launch may write."""

    def __init__(self, entry, contents, outs, call, make=None, reserve=None, outside=None, verify=None):
        self.entry, self.contents, self.outs, self.call = entry, contents, outs, call
        self.make = make or (lambda eng: None)
        self.reserve = reserve or (lambda eng, h: None)
        self.outside = outside
        self.verify = verify             # verify(want): that the eager results show the contents are what they claim
        for c in contents[1:]:
            assert {k: as_bytes(v).size for k, v in c.items()} == {k: as_bytes(v).size for k, v in contents[0].items()}

    def buffers(self, content):
        B = {k: dev_of(v) for k, v in content.items()}
        B.update({k: dev_fill(nbytes_of(*ds)) for k, ds in self.outs.items()})
        return B

    def results(self, B):
        return {k: download(B[k], dt, shape) for k, (dt, shape) in self.outs.items()}


def stft_case(n_fft, hop, F=5):
    n = hop * (F - 1) + n_fft
    return Stateless("jdsp_stft_i16_dev", [{"pcm": noise_i16(100 + i + hop, n)} for i in range(3)],
                     {"spec": (np.complex64, (F, n_fft))},
                     lambda eng, h, B: lib().jdsp_stft_i16_dev(eng._h, vp(B["pcm"]), F, n_fft, hop, vp(B["spec"])))


def stft_half_case(F=5):
    return Stateless("jdsp_stft_half_i16_dev", [{"pcm": noise_i16(120 + i, 512 * (F - 1) + 1024)} for i in range(3)],
                     {"spec": (np.complex64, (F, 513))},
                     lambda eng, h, B: lib().jdsp_stft_half_i16_dev(eng._h, vp(B["pcm"]), F, vp(B["spec"]), 513))


def stft_f64_case(F=5):
    return Stateless("jdsp_stft_i16_f64_dev", [{"pcm": noise_i16(130 + i, 512 * (F - 1) + 1024)} for i in range(3)],
                     {"spec": (np.complex128, (F, 1024))},
                     lambda eng, h, B: lib().jdsp_stft_i16_f64_dev(eng._h, vp(B["pcm"]), F, 1024, 512, vp(B["spec"])))


def _span_mask(size, offs, spans):
    """True where no utterance's span lies"""
    out = np.ones(size, bool)
    for a, s in zip(offs, spans):
        out[int(a):int(a) + int(s)] = False
    return out


def stft_half_batch_case(hop=512, pitch=520, spare=2):
    from test_stft_batch_gpu import Batch
    bs = [Batch(np.random.default_rng(140 + i), hop, fr) for i, fr in enumerate(dealt(1024 // hop))]
    contents = [{"pcm": b.pcm, "sample_first": b.offs[:-1], "frame_first": b.first} for b in bs]
    rows = N_FRAMES + spare
    keep = np.ones((rows, pitch), bool)
    keep[:N_FRAMES, :513] = False
    return Stateless("jdsp_stft_half_batch_dev", contents, {"spec": (np.complex64, (rows, pitch))},
                     lambda eng, h, B: lib().jdsp_stft_half_batch_dev(eng._h, vp(B["pcm"]), vp(B["sample_first"]),
                                                                      vp(B["frame_first"]), N_UTTS, N_FRAMES, hop,
                                                                      vp(B["spec"]), pitch),
                     outside=lambda c: {"spec": keep})


def istft_batch_case(n, hop, layout):
    from test_istft_batch_gpu import Batch, cfg_of
    bs = [Batch(np.random.default_rng(150 + i + n), n, hop, layout, fr) for i, fr in enumerate(dealt(n // hop))]
    size, pitch = bs[0].size, bs[0].pitch
    assert all(b.size == size and b.total == N_FRAMES for b in bs)
    contents = [{"spec": b.spec, "sample_first": b.offs[:-1], "frame_first": b.first} for b in bs]
    masks = {c["sample_first"].tobytes(): _span_mask(size, b.offs[:-1], b.spans) for c, b in zip(contents, bs)}
    return Stateless("jdsp_istft_batch_dev", contents, {"out_i16": (np.int16, (size,)), "out_f32": (np.float32, (size,))},
                     lambda eng, h, B: lib().jdsp_istft_batch_dev(h._h, vp(B["spec"]), pitch, vp(B["sample_first"]),
                                                                  vp(B["frame_first"]), N_UTTS, N_FRAMES, vp(B["out_i16"]),
                                                                  vp(B["out_f32"])),
                     make=lambda eng: eng.istft(**cfg_of(n, hop, layout)),
                     outside=lambda c: dict.fromkeys(("out_i16", "out_f32"), masks[c["sample_first"].tobytes()]))


def stftmask_batch_case(hop=256, kind="real"):
    from test_stftmask_batch_gpu import Batch
    from test_stftmask_gpu import BINS, cfg_of, stream_combo
    bs = [Batch(np.random.default_rng(160 + i), kind, hop, fr) for i, fr in enumerate(dealt(1024 // hop))]
    size = bs[0].pcm.size
    assert all(b.pcm.size == size and int(b.first[-1]) == N_FRAMES and b.mask.shape == (N_FRAMES, BINS) for b in bs)
    contents = [{"pcm": b.pcm, "mask": b.mask, "sample_first": b.offs[:-1], "frame_first": b.first} for b in bs]
    masks = {c["sample_first"].tobytes(): _span_mask(size, b.offs[:-1], b.spans) for c, b in zip(contents, bs)}
    return Stateless("jdsp_stftmask_batch_dev", contents,
                     {"out_i16": (np.int16, (size,)), "out_f32": (np.float32, (size,))},
                     lambda eng, h, B: lib().jdsp_stftmask_batch_dev(h._h, vp(B["pcm"]), vp(B["mask"]), BINS,
                                                                     vp(B["sample_first"]), vp(B["frame_first"]), N_UTTS,
                                                                     N_FRAMES, vp(B["out_i16"]), vp(B["out_f32"])),
                     make=lambda eng: eng.stft_mask(**cfg_of(hop, kind, stream_combo(hop))),
                     outside=lambda c: dict.fromkeys(("out_i16", "out_f32"), masks[c["sample_first"].tobytes()]))


def denoise_batch_case(mode=0):
    """Three utterances of 40 blocks in all, each a loud block, ten quiet ones (the run length at which the estimate is
    latched) and loud ones after them; the lengths are dealt anew every time."""
    from test_denoise_batch_gpu import B, Batch, loud, quiet
    bs = []
    for i, lens in enumerate([(14, 11, 15), (11, 15, 14), (15, 14, 11)]):
        rng = np.random.default_rng(170 + i)
        bs.append(Batch([np.concatenate([loud(rng, 1), quiet(rng, 10), loud(rng, n - 11)]) for n in lens], gap=2))
    size, total = bs[0].n_samples, 40
    assert all(b.n_samples == size and b.n_total == total for b in bs)
    contents = [{"pcm": b.pcm, "sample_first": b.sample_first, "block_first": b.block_first} for b in bs]

    def outside(c):
        keep = np.ones(size, bool)
        first, blocks = c["sample_first"], np.diff(c["block_first"])
        for s, nb in zip(first, blocks):
            keep[int(s) + B:int(s) + (int(nb) - 1) * B] = False
        return {"out": keep, "precast": keep}

    def verify(want):
        for w in want:                                             # estimation events occurred in every utterance
            assert w["noise_last"].any(axis=1).all(), "an utterance latched no estimate: the input is wrong"
            assert set(np.unique(w["flags"])) == {0, 1}

    return Stateless("jdsp_denoise_batch_dev", contents,
                     {"out": (np.int16, (size,)), "precast": (np.float32, (size,)), "flags": (np.uint8, (total,)),
                      "noise_last": (np.float32, (3, 1024))},
                     lambda eng, h, Bf: lib().jdsp_denoise_batch_dev(h._h, vp(Bf["pcm"]), vp(Bf["sample_first"]),
                                                                     vp(Bf["block_first"]), 3, total, vp(Bf["out"]),
                                                                     vp(Bf["precast"]), vp(Bf["flags"]), vp(Bf["noise_last"])),
                     make=lambda eng: eng.denoiser(mode),
                     reserve=lambda eng, h: ok(eng, lib().jdsp_denoise_batch_reserve(h._h, total, 3), "batch_reserve"),
                     outside=outside, verify=verify)


def mfcc_case(kw, n, fs, n_cep, n_bins, kinds, least, F=16):
    """Frames that the FP64 redo pass takes (quiet coloured frames 35 dB under a loud neighbour, mfcc_fp32_ref's cases
    of the kinds `kinds`), then white frames that it does not, then redo-heavy frames again: the redo list is
    non-empty, empty, non-empty.  Which frames took the pass shows in the result itself: the FP64 pass lands within
    1e-13 of the FP64 oracle, the FP32 kernels between 2e-7 and 2e-6 of it, so 1e-10 tells them apart.  `least` frames
    of the first and the third content must have taken it (measured: all 16 on the pair kernel; 12 and 14 of 16 on the
    native configuration, whose kernel judges every pair by its own frames), none of the white ones."""
    import mfcc_fp32_ref as R
    quiet = [c for c in R.cases(n, fs) if c["db"] == 35 and c["kind"] in kinds]
    assert len(quiet) >= F
    rng = np.random.default_rng(180)
    sets = [R.frames_of(quiet[:F // 2]), np.stack([R.white(rng, n, 3000.0) for _ in range(F)]),
            R.frames_of(quiet[F // 2:F])]
    start = n * np.arange(F, dtype=np.int64)
    contents = [{"pcm": np.ascontiguousarray(s, np.int16).reshape(-1), "frame_start": start} for s in sets]

    def verify(want):
        import oracle_lib
        oracle = oracle_lib.load_oracle()
        ocfg = oracle.mfcc_cfg(n_bins=n_bins, **kw)
        took = []
        for s, w in zip(sets, want):
            ref = np.stack([oracle.mfcc_frames(ocfg, np.ascontiguousarray(fr, np.int16), 1)[0] for fr in s])
            err = (np.abs(w["feats"] - ref) / np.abs(ref).max(axis=1, keepdims=True)).max(axis=1)
            took.append(int((err < 1e-10).sum()))
        print("frames the FP64 pass took, of %d: %s" % (F, took))
        assert took[0] >= least and took[1] == 0 and took[2] >= least, took

    return Stateless("jdsp_mfcc_frames_dev", contents, {"feats": (np.float64, (F, n_cep))},
                     lambda eng, h, B: lib().jdsp_mfcc_frames_dev(h._h, vp(B["pcm"]), vp(B["frame_start"]), F, vp(B["feats"])),
                     make=lambda eng: eng.mfcc(**kw), verify=verify)


def _voiced(seed, n, f0):
    t = np.arange(n)
    x = 6000.0 * np.sin(2 * np.pi * f0 * t / 16000.0) + np.random.default_rng(seed).normal(0, 800.0, n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _blocks(block, nb=3):
    return [{"pcm": _voiced(190 + i, block * nb, 110.0 + 45.0 * i), "prev": _voiced(195 + i, block, 140.0 + 30.0 * i)}
            for i in range(3)]


def pitch_autocorr_case(nb=3):
    return Stateless("jdsp_pitch_autocorr_dev", _blocks(512, nb),
                     {"arg": (np.int32, (nb,)), "rmax": (np.float32, (nb,)), "autocorr": (np.float32, (nb, 512))},
                     lambda eng, h, B: lib().jdsp_pitch_autocorr_dev(eng._h, vp(B["pcm"]), nb, vp(B["prev"]), vp(B["arg"]),
                                                                     vp(B["rmax"]), vp(B["autocorr"])))


def pitch_lag_case(method, nb=3):
    return Stateless("jdsp_pitch_lag_dev", _blocks(512, nb),
                     {"arg": (np.int32, (nb,)), "value": (np.float64, (nb,)), "curve": (np.float64, (nb, 512))},
                     lambda eng, h, B: lib().jdsp_pitch_lag_dev(eng._h, method, vp(B["pcm"]), nb, vp(B["prev"]),
                                                                vp(B["arg"]), vp(B["value"]), vp(B["curve"])))


def lpc_case(block=256, order=12, nb=3):
    return Stateless("jdsp_lpc_dev", _blocks(block, nb),
                     {"autocorr": (np.float64, (nb, order + 1)), "lpc": (np.float64, (nb, order))},
                     lambda eng, h, B: lib().jdsp_lpc_dev(eng._h, vp(B["pcm"]), nb, block, order, vp(B["prev"]),
                                                          vp(B["autocorr"]), vp(B["lpc"])))


def gmm_case(n_classes=25):
    import gmm_cases as gc
    classes = gc.gmm_records(11, n_classes)
    lens = [[0, 1, 30, 9], [30, 0, 9, 1], [9, 1, 0, 30]]
    contents = [{"feats": gc.vectors(200 + i, 40), "utt_first": gc.offsets(ln)} for i, ln in enumerate(lens)]
    return Stateless("jdsp_gmm_score_dev", contents, {"scores": (np.float64, (4, n_classes)), "best": (np.int32, (4,))},
                     lambda eng, h, B: lib().jdsp_gmm_score_dev(h._h, vp(B["feats"]), 40, vp(B["utt_first"]), 4,
                                                                vp(B["scores"]), vp(B["best"])),
                     make=lambda eng: eng.gmm(classes))


def hmm_case():
    import gmm_cases as gc
    models = gc.hmm_records_finite(21, 2)
    contents = []
    for i, lens in enumerate([[5, 12, 8], [12, 8, 5], [8, 5, 12]]):
        x = np.concatenate([gc.vectors_near(210 + 3 * i + u, n, models["gMMParam"][u % 2, (2 * u + i) % 6])
                            for u, n in enumerate(lens)])
        contents.append({"feats": x, "utt_first": gc.offsets(lens)})
    return Stateless("jdsp_hmm_viterbi_dev", contents,
                     {"scores": (np.float64, (3, 2)), "best": (np.int32, (3,)), "path": (np.int32, (2, 25)),
                      "trellis": (np.float64, (2, 6, 25))},
                     lambda eng, h, B: lib().jdsp_hmm_viterbi_dev(h._h, vp(B["feats"]), 25, vp(B["utt_first"]), 3,
                                                                  vp(B["scores"]), vp(B["best"]), vp(B["path"]),
                                                                  vp(B["trellis"])),
                     make=lambda eng: eng.hmm(models),
                     reserve=lambda eng, h: ok(eng, lib().jdsp_hmm_reserve(h._h, 25), "jdsp_hmm_reserve"))


def fft_case(n=512, batch=3):
    def content(i):
        rng = np.random.default_rng(220 + i)
        return {"x": (rng.normal(0, 1000.0, (batch, n)) + 1j * rng.normal(0, 1000.0, (batch, n))).astype(np.complex128)}
    return Stateless("jdsp_fft_process_f64_dev", [content(i) for i in range(3)], {"y": (np.complex128, (batch, n))},
                     lambda eng, h, B: lib().jdsp_fft_process_f64_dev(eng._h, vp(B["x"]), vp(B["y"]), n, batch, 1))


KW4 = dict(win_len=400, hop=160, n_fft=512, n_chan=40, n_cep=13, half_rate=8000.0)      # BASELINE config 4

# id -> builder; every entry of class S appears here and in no other table
STATELESS = {
    "stft_i16-1024-512": lambda: stft_case(1024, 512),
    "stft_i16-512-256": lambda: stft_case(512, 256),
    "stft_i16-1024-160": lambda: stft_case(1024, 160),
    "stft_half_i16": stft_half_case,
    "stft_i16_f64": stft_f64_case,
    "stft_half_batch": stft_half_batch_case,
    "istft_batch-1024-256-full": lambda: istft_batch_case(1024, 256, "full"),
    "istft_batch-512-128-half": lambda: istft_batch_case(512, 128, "half"),
    "stftmask_batch-256-real": stftmask_batch_case,
    "denoise_batch-ss": denoise_batch_case,
    "mfcc_frames-native": lambda: mfcc_case({}, 1024, 44100.0, 12, 512, ("highpass", "tone"), 8),
    "mfcc_frames-config4": lambda: mfcc_case(KW4, 400, 16000.0, 13, 256, ("vowel120", "vowel180"), 16),
    "pitch_autocorr": pitch_autocorr_case,
    "pitch_lag-amdf": lambda: pitch_lag_case(2),
    "pitch_lag-acf": lambda: pitch_lag_case(3),
    "lpc-256-12": lpc_case,
    "gmm_score-25": gmm_case,
    "hmm_viterbi": hmm_case,
    "fft_process_f64-512": fft_case,
}


# ---- class D: the live streams --------------------------------------------------------------------------------------
N_CHUNKS = 4


def live_plan(R, n_streams=6):
    """Deliveries of N_CHUNKS chunks and 2 R + 5 frames each, as (stream, frames) lists: other stream sets in another
    order every time (so every stream is absent from some), a chunk of no frames and a chunk of one frame in each,
    stream n_streams - 1 never fed.  With one stream: n_chunks is 1 and every delivery has 2 R + 5 frames."""
    T = 2 * R + 5
    if n_streams == 1:
        return [[(0, T)] for _ in range(5)]
    return [[(2, 0), (0, T - 4), (4, 1), (1, 3)],
            [(1, 1), (4, R), (0, 0), (3, T - 1 - R)],
            [(3, 2), (2, 1), (1, 0), (0, T - 3)],
            [(4, T - R - 1), (1, R), (2, 0), (0, 1)],
            [(0, 0), (3, 1), (2, T - 3), (4, 2)]]


class Live:
    """The buffers of one captured delivery on a live-stream handle and the calls on them.  kind: "stftmask" or "istft";
    st: the Streams object of that handle's own test module (its call() packs a delivery, its take() hands the outputs
    to the streams and checks the sentinels, its check() compares with the single-stream reference)."""

    def __init__(self, eng, kind, h, st, n_chunks, n_total, pitch, cap):
        import torch
        self.eng, self.kind, self.h, self.st = eng, kind, h, st
        self.n_chunks, self.n_total, self.pitch, self.cap = n_chunks, n_total, pitch, cap
        self.n, self.hop = h.n_fft, h.hop
        z64 = np.zeros(n_chunks + 1, np.int64)
        self.ids, self.first, self.ff = dev_of(z64[:-1]), dev_of(z64[:-1]), dev_of(z64)
        if kind == "stftmask":
            self.pcm = dev_of(np.full(cap, 32767, np.int16))
            elem = 8 if st.kind == "complex" else 4
            self.rows = dev_fill(n_total * pitch * elem)
        else:
            self.pcm = None
            self.rows = dev_fill(n_total * pitch * 8)
        self.out_i, self.out_f = dev_fill(cap * 2), dev_fill(cap * 4)
        tail = self.n - self.hop
        self.n_ids = st_n = len(st.totals)
        self.f_ids = dev_of(np.arange(st_n, dtype=np.int64))
        self.f_first = dev_of(np.arange(st_n, dtype=np.int64) * tail)
        self.f_i, self.f_f = dev_fill(st_n * tail * 2), dev_fill(st_n * tail * 4)
        self.r_ids = dev_of(np.zeros(1, np.int64))
        self.torch = torch

    def c(self, name):
        return self.h._c(name)

    def deliver(self):
        """the C call of one delivery on the captured buffers"""
        a = (vp(self.ids), vp(self.first), vp(self.ff), self.n_chunks, self.n_total, vp(self.out_i), vp(self.out_f))
        if self.kind == "stftmask":
            rc = self.c("_streams_dev")(self.h._h, vp(self.pcm), vp(self.rows), self.pitch, *a)
        else:
            rc = self.c("_streams_dev")(self.h._h, vp(self.rows), self.pitch, *a)
        ok(self.eng, rc, "_streams_dev")

    def flush(self):
        ok(self.eng, self.c("_streams_flush_dev")(self.h._h, vp(self.f_ids), vp(self.f_first), self.n_ids, vp(self.f_i),
                                                  vp(self.f_f)), "_streams_flush_dev")

    def reset_one(self):
        ok(self.eng, self.c("_streams_reset_dev")(self.h._h, vp(self.r_ids), 1), "_streams_reset_dev")

    def load(self, chunks):
        """a delivery's content into the captured buffers; the outputs back to the sentinel"""
        packed = self.st.call(chunks)
        if self.kind == "stftmask":
            pcm, rows, ids, counts, first = packed
            assert pcm.size <= self.cap
            full = np.full(self.cap, 32767, np.int16)
            full[:pcm.size] = pcm
            upload(self.pcm, full)
        else:
            rows, ids, counts, first, size = packed
            assert size <= self.cap
        assert len(chunks) == self.n_chunks and int(counts.sum()) == self.n_total and rows.shape == (self.n_total, self.pitch)
        upload(self.rows, rows)
        upload(self.ids, ids)
        upload(self.first, first)
        upload(self.ff, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
        self.out_i.fill_(FILL)
        self.out_f.fill_(FILL)
        return first

    def take(self, chunks, first, what):
        """after the replay: the outputs to their streams; the take() of the handle's module checks its own sentinels,
        so the FILL bytes are turned into those outside the written ranges first"""
        from test_stftmask_streams_gpu import SENT_F, SENT_I
        oi, of = download(self.out_i, np.int16), download(self.out_f, np.float32)
        covered = np.zeros(oi.size, bool)
        for (s, f), a in zip(chunks, first):
            covered[int(a):int(a) + self.hop * f] = True
        assert np.all(oi[~covered] == sentinel(np.int16)), (what, "int16 outside the written ranges")
        assert np.all(of[~covered].view(np.int32) == sentinel(np.int32)), (what, "float32 outside the written ranges")
        oi[~covered], of[~covered] = SENT_I, SENT_F
        self.st.take(chunks, first, oi, of, what)

    def flushed(self):
        tail = self.n - self.hop
        return (download(self.f_i, np.int16, (self.n_ids, tail)), download(self.f_f, np.float32, (self.n_ids, tail)))


def live_case(eng, kind, cfg, n_streams, seed, totals):
    """(handle, Streams, Live, reference): a handle with n_streams live streams, warm for one delivery's scalars"""
    R = cfg["n_fft"] // cfg["hop"]
    n_chunks = N_CHUNKS if n_streams > 1 else 1
    T = 2 * R + 5
    n, hop = cfg["n_fft"], cfg["hop"]
    cap = hop * T + n_chunks * (n + 32) + 64
    rng = np.random.default_rng(seed)
    if kind == "stftmask":
        import test_stftmask_streams_gpu as M
        st = M.Streams(rng, cfg["mask_kind"], hop, totals)
        h, pitch = eng.stft_mask(**cfg), M.BINS
    else:
        import test_istft_streams_gpu as M
        st = M.Streams(rng, n, hop, cfg["layout"], totals)
        h, pitch = eng.istft(**cfg), st.pitch
    ref = st.reference(eng, cfg)
    h.open_streams(n_streams)
    return h, st, Live(eng, kind, h, st, n_chunks, T, pitch, cap), ref


def totals_of(plans, n_streams):
    return [sum(f for chunks in plans for s, f in chunks if s == k) for k in range(n_streams)]


# ---- class H: host-carried state -----------------------------------------------------------------------------------
class Carried:
    """One handle whose stream position lives on the host.  sizes: the calls of the whole stream, in blocks or frames;
    graph: (first, last + 1) of the calls captured into ONE graph.  Every call has buffers of its own, made before the
    capture.  issue(k) enqueues call k and returns what is needed to read its outputs; read(k, info) -> list of numpy
    arrays; state() -> list of numpy arrays (the getters); finish() enqueues the flush, if the handle has one."""

    def __init__(self, eng):
        self.eng = eng

    def run(self, sizes, graph=None):
        """the stream, call after call: eagerly, or with the calls graph[0] .. graph[1] - 1 captured and replayed once"""
        import torch
        self.prepare(sizes)
        infos = {}
        k = 0
        while k < len(sizes):
            if graph and k == graph[0]:
                def body():
                    for j in range(graph[0], graph[1]):
                        infos[j] = self.issue(j)
                g = capture(self.eng, body)
                g.replay()                                     # once, where the handle stood at capture
                torch.cuda.synchronize()
                k = graph[1]
                continue
            self.eng._use_torch_stream()
            infos[k] = self.issue(k)
            k += 1
        self.eng._use_torch_stream()
        self.finish()
        torch.cuda.synchronize()
        outs = [a for k in range(len(sizes)) for a in self.read(k, infos[k])] + self.read_finish()
        return outs, self.state()

    def finish(self):
        pass

    def read_finish(self):
        return []

    def state(self):
        return []


def same_bytes(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b)) \
        and len(a) == len(b)
