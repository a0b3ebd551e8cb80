#!/usr/bin/env python3
"""Secondary figures: the chains downstream of the STFT, each timed with HIP
events on the stream it runs on, inputs resident in HBM.  One JSON line per chain.

    python tools/bench_chains.py [--iters 20]

These are reported next to, never instead of, bench.py's headline metric."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jeicyboodsp_amd  # noqa: E402
import oracle_lib  # noqa: E402  (CPU checker: timed here as the per-chain CPU baseline, never used by the product)

HBM_PEAK = 8000.0       # GB/s
FP32_PEAK = 157.3       # TFLOP/s vector
TD_CLOCK_GHZ = 2.4      # peak engine clock: the issue bound of the time-domain legs counts one lane-instruction per lane and clock
TD_TERMS_ALL = sum(1024 - k for k in range(512))            # 393,472 lag terms of a frame, all 512 lags
TD_TERMS_SEARCH = sum(1024 - k for k in range(101, 512))    # 295,098: the lags the arg search reads


def timed(fn, iters, rounds=5, spin_ms=60.0):
    """Median over `rounds` of the mean launch time of `iters` back-to-back calls, after `spin_ms` of the same
    calls: a GPU that has idled needs tens of milliseconds of load to reach its sustained clocks
    (profiles/r01_bench_warmup_sweep.txt)."""
    import time
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < spin_ms:
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / iters)
    return statistics.median(ts)


def timed_alternated(fns, iters, rounds=5, spin_ms=60.0):
    """timed() for several callables in ONE sequence of alternated rounds: every round times each of them in turn
    (iters[i] back-to-back calls of fns[i]), so a drift of the clocks or of the box falls on all of them alike.
    Returns their medians."""
    import time
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < spin_ms:
        fns[0]()
        torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters[i]):
                fn()
            b.record()
            torch.cuda.synchronize()
            ts[i].append(a.elapsed_time(b) / iters[i])
    return [statistics.median(t) for t in ts]


def cpu_rate(fn, units):
    """units/s of the CPU oracle (FP64, one thread, structured like the reference) on a bounded sample."""
    import time
    fn()
    t0 = time.perf_counter()
    n = 0
    while time.perf_counter() - t0 < 1.5:
        fn()
        n += 1
    return units * n / (time.perf_counter() - t0)


def pcm_of(rng, n, sigma=3000.0):
    return np.clip(np.rint(rng.normal(0, sigma, n)), -32768, 32767).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="")
    ap.add_argument("--warm", action="store_true",
                    help="every call re-reads ONE input buffer (it then lives in the 256 MiB Infinity Cache); default: the calls "
                         "rotate over 6 copies of the input (>= 256 MiB for the 65,536-block chains), so the PCM comes from HBM")
    ap.add_argument("--denoise-k", type=int, default=0, help="denoise blocks_per_wave (0 = auto: one round of resident waves)")
    a = ap.parse_args()
    eng = jeicyboodsp_amd.Engine(0)
    orc = oracle_lib.load_oracle()
    rng = np.random.default_rng(0)
    out = []

    def report(name, ms, units, unit_name, bytes_per_unit, flops_per_unit, note="", cpu=None, inp=None):
        rate = units / (ms * 1e-3)
        gbs = rate * bytes_per_unit / 1e9
        tf = rate * flops_per_unit / 1e12
        line = {"chain": name, "ms": ms, "units": units, "unit": unit_name, "rate_per_s": rate,
                "input": inp or ("re-read from one buffer (cache-resident)" if a.warm else "rotated over 6 copies (from HBM) where the chain's input is a PCM stream"),
                "algorithmic_GBps": gbs, "hbm_frac": gbs / HBM_PEAK, "fft_TFLOPs": tf, "fp32_vector_frac": tf / FP32_PEAK,
                "note": note}
        if cpu is not None:
            line["cpu_baseline"] = {"value": cpu, "unit": unit_name + "/s", "cores": 1, "kind": "port"}
        out.append(line)
        print(json.dumps(line), flush=True)

    B = 65536
    want = set(a.only.split(",")) if a.only else None

    class rot:
        """6 device copies of an input, handed out in turn (cold input); --warm: the one buffer every time."""

        def __init__(self, t):
            self.bufs = [t] if a.warm else [t] + [t.clone() for _ in range(5)]
            self.i = 0

        def __call__(self):
            self.i += 1
            return self.bufs[self.i % len(self.bufs)]

    def on(n):
        return want is None or n in want

    if on("stft_half"):
        x = torch.from_numpy(pcm_of(rng, 512 * (B + 1))).cuda()
        for pitch in (513, 514, 516, 520, 528, 576, 1024):
            hs = torch.empty((B, pitch), dtype=torch.complex64, device="cuda")
            ms = timed(lambda: eng.stft_half(x, B, out=hs, pitch=pitch), a.iters)
            report(f"stft_half_spectrum_513_bins_pitch{pitch}", ms, B, "frames", 1024 + 4104, 5 * 512 * 9 + 512 * 14,
                   "extra: bins 0..512 only (5,128 algorithmic bytes per frame); the headline keeps all 1024 bins")
    if on("stft_f64"):
        x = torch.from_numpy(pcm_of(rng, 512 * (B + 1))).cuda()
        xr = rot(x)
        o64 = torch.empty((B, 1024), dtype=torch.complex128, device="cuda")
        ms = timed(lambda: eng.stft_f64(xr(), B, 512, out=o64), a.iters)
        report("stft_1024_hop512_fp64", ms, B, "frames", 1024 + 16384, 5 * 512 * 9 + 512 * 14,
               "the headline analysis in the reference's own precision: FP64 window and transform, complex128 full spectrum "
               "(17,408 algorithmic bytes per frame); flops are FP64")
    if on("istft"):
        # STFT synthesis (jdsp_istft): 65,536 frames per call, spectra rotated over 6 copies (from HBM)
        for name, n, hop, layout, pitch, nbytes in (("istft_1024_hop512_full", 1024, 512, "full", 1024, 8192 + 1024),
                                                    ("istft_1024_hop512_half_pitch513", 1024, 512, "half", 513, 4104 + 1024),
                                                    ("istft_1024_hop256_full", 1024, 256, "full", 1024, 8192 + 1024),
                                                    ("istft_512_hop256_full", 512, 256, "full", 512, 4096 + 512)):
            gen = torch.Generator(device="cuda").manual_seed(n + hop)
            spec = torch.randn((B, pitch), dtype=torch.complex64, device="cuda", generator=gen) * 3000.0 * np.sqrt(n)
            sr = rot(spec)
            ist = eng.istft(n_fft=n, hop=hop, layout=layout)
            o16 = torch.empty(B * hop, dtype=torch.int16, device="cuda")
            ms = timed(lambda: ist.process(sr(), out=o16), a.iters)
            report(name, ms, B, "frames", nbytes, 5 * (n // 2) * 9 + (n // 2) * 14,
                   "STFT synthesis: Hermitian pairing, one 512-point inverse per frame, overlap-add, int16 out "
                   "(%d algorithmic bytes per frame; the halo frames a wave recomputes are not counted)" % nbytes)
            ist.close()
            del spec, sr
    if on("stftmask"):
        # Fused STFT masking (jdsp_stftmask) against the unfused route timed the same way: analysis to HBM -> in-place
        # torch multiply -> synthesis.  65,536 frames per call; PCM and mask rows rotate over 6 copies (from HBM).
        flops = 2 * (5 * 512 * 9 + 512 * 14)
        for name, hop, kind in (("stftmask_1024_hop512_real", 512, "real"), ("stftmask_1024_hop512_complex", 512, "complex"),
                                ("stftmask_1024_hop256_real", 256, "real")):
            cpx = kind == "complex"
            nbytes = 2 * hop + 513 * (8 if cpx else 4) + 2 * hop
            gen = torch.Generator(device="cuda").manual_seed(hop + cpx)
            x = torch.from_numpy(pcm_of(rng, hop * (B - 1) + 1024)).cuda()
            mask = torch.rand((B, 513), dtype=torch.float32, device="cuda", generator=gen) * 1.5
            if cpx:
                mask = torch.polar(mask, torch.rand((B, 513), dtype=torch.float32, device="cuda", generator=gen) * 6.2831853)
            xr, mr = rot(x), rot(mask)
            o16 = torch.empty(B * hop, dtype=torch.int16, device="cuda")
            sm = eng.stft_mask(n_fft=1024, hop=hop, analysis_window="hamming", synthesis_window="none", normalise=0,
                               mask_kind=kind)
            ms = timed(lambda: sm.process(xr(), mr(), B, out=o16), a.iters)
            report(name, ms, B, "frames", nbytes, flops,
                   "fused analysis -> %s mask -> synthesis, int16 in and out, no spectrum in memory (%d algorithmic bytes "
                   "per frame: %d PCM + %d mask + %d out; the halo frames a wave recomputes are not counted)"
                   % (kind, nbytes, 2 * hop, nbytes - 4 * hop, 2 * hop))
            sm.close()
            # the unfused route on the same inputs: the spectrum goes to HBM, is multiplied there and read back
            half = hop == 512
            if half:
                spec = torch.empty((B, 513), dtype=torch.complex64, device="cuda")
                full_mask = None
                analyse = lambda: eng.stft_half(xr(), B, out=spec, pitch=513)  # noqa: E731
            else:
                spec = torch.empty((B, 1024), dtype=torch.complex64, device="cuda")
                full_mask = rot(torch.cat([mask, mask[:, 1:512].flip(1)], dim=1).contiguous())
                analyse = lambda: eng.stft(xr(), B, 1024, hop, out=spec)  # noqa: E731
            ist = eng.istft(n_fft=1024, hop=hop, layout="half" if half else "full")

            def unfused():
                analyse()
                spec.mul_(mr() if half else full_mask())
                ist.process(spec, out=o16)

            ms_u = timed(unfused, a.iters)
            ubytes = 2 * hop + 3 * spec.shape[1] * 8 + spec.shape[1] * (8 if cpx else 4) + 2 * hop
            report(name.replace("stftmask_", "unfused_stft_mul_istft_"), ms_u, B, "frames", ubytes, flops,
                   "the same work as three launches through a %d-byte-per-frame spectrum workspace (%s): %.3f ms against "
                   "%.3f ms fused on the same box in the same process, ratio %.2f"
                   % (spec.shape[1] * 8, "stft_half pitch 513 -> torch mul_ -> istft half" if half
                      else "stft full -> torch mul_ -> istft full", ms_u, ms, ms_u / ms))
            ist.close()
            del x, mask, xr, mr, spec, full_mask, o16
    if on("stftmask_batch"):
        # Batched fused STFT masking (jdsp_stftmask_batch_dev): 10,000 ragged utterances (seeded, 100..500 frames at hop
        # 512: the same PCM is 200..1000 frames at hop 256), real mask, timed three ways in this process: (a) the batch
        # entry, one launch; (b) process + flush per utterance on one handle, 20,000 launches, the C entries called
        # through ctypes with every pointer computed beforehand; (c) ONE stream of the same total frame count over the
        # same buffers, the floor.  The PCM (GBs) and the mask rows (more GBs) are far past the 256 MiB Infinity Cache, so
        # one copy of each already comes from HBM.
        import ctypes as C
        from jeicyboodsp_amd import sharding
        from jeicyboodsp_amd._lib import lib as L
        flops = 2 * (5 * 512 * 9 + 512 * 14)
        lens = 2 * np.random.default_rng(10000).integers((1024 + 99 * 512) // 2, (1024 + 500 * 512) // 2, 10000)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        gen = torch.Generator(device="cuda").manual_seed(10000)
        x = (torch.randn(int(offs[-1]), device="cuda", generator=gen) * 3000.0).clamp_(-32768, 32767).to(torch.int16)
        for hop in (512, 256):
            counts, first = sharding.stftmask_batch_layout(offs, 1024, hop)
            total = int(first[-1])
            mask = torch.rand((total, 513), dtype=torch.float32, device="cuda", generator=gen) * 1.5
            o16 = torch.empty(x.numel(), dtype=torch.int16, device="cuda")
            sm = eng.stft_mask(n_fft=1024, hop=hop, analysis_window="hann", synthesis_window="hann", normalise=1)
            nbytes = 2 * hop + 513 * 4 + 2 * hop
            what = "10,000 ragged utterances, %d frames (%d..%d each), hop %d, real mask" % (total, counts.min(), counts.max(), hop)
            inp = "one copy: %.1f GB of PCM and %.1f GB of mask rows per call (from HBM)" % (2e-9 * x.numel(), 4e-9 * mask.numel())
            ms_a = timed(lambda: sm.process_batch(x, mask, offs, out=o16), max(a.iters // 4, 3))
            ms_c = timed(lambda: sm.process(x, mask, total, out=o16), max(a.iters // 4, 3))
            sm.flush()
            # (b): the argument lists of the 10,000 process_dev and flush_dev calls
            h, px, pm, po = sm._h, x.data_ptr(), mask.data_ptr(), o16.data_ptr()
            calls = []
            for u in range(len(counts)):
                s, f = int(offs[u]), int(counts[u])
                calls.append(((h, C.c_void_p(px + 2 * s), C.c_void_p(pm + 4 * 513 * int(first[u])), 513, f,
                               C.c_void_p(po + 2 * s), None), (h, C.c_void_p(po + 2 * (s + hop * f)), None)))
            eng._use_torch_stream()

            def loop():
                for p, fl in calls:
                    L.jdsp_stftmask_process_dev(*p)
                    L.jdsp_stftmask_flush_dev(*fl)

            ms_b = timed(loop, 1, rounds=3, spin_ms=0.0)
            report("stftmask_batch_1024_hop%d_real" % hop, ms_a, total, "frames", nbytes, flops,
                   "(a) jdsp_stftmask_batch_dev, one launch: %s; %.2f x the single stream (c), %.3f of the per-utterance "
                   "loop (b)" % (what, ms_a / ms_c, ms_a / ms_b), inp=inp)
            report("stftmask_batch_1024_hop%d_real_per_utterance_loop" % hop, ms_b, total, "frames", nbytes, flops,
                   "(b) the same batch as 10,000 x (jdsp_stftmask_process_dev + jdsp_stftmask_flush_dev) on one handle, "
                   "from ctypes with precomputed arguments: %.1f x the batch entry" % (ms_b / ms_a), inp=inp)
            report("stftmask_batch_1024_hop%d_real_single_stream" % hop, ms_c, total, "frames", nbytes, flops,
                   "(c) the floor: ONE stream of the same %d frames over the same buffers, one jdsp_stftmask_process_dev" % total,
                   inp=inp)
            sm.close()
            del mask, o16
        del x
    if on("stft_half_batch") or on("istft_batch"):
        # The analysis and synthesis ends of the ragged-batch pipeline (jdsp_stft_half_batch_dev, jdsp_istft_batch_dev) on
        # the stftmask_batch leg's 10,000 seeded utterances, half layout, pitch 520, Hann / Hann.  Each is timed three ways
        # in this process, in alternated rounds: (a) the batch entry, one launch; (b) the per-utterance loop on the
        # single-stream _dev entries, the C entries called through ctypes with every pointer computed beforehand; (c) ONE
        # stream of the same total frame count over the same buffers.  Analysis (b) is jdsp_stft_i16_dev per utterance,
        # the entry the batch rows are bit-identical to, into the utterance's rows of a full-spectrum tensor (the
        # half-spectrum single-stream entry wants 16-byte aligned PCM, which an utterance at an even offset is not);
        # analysis (c) is jdsp_stft_half_i16_dev at hop 512 and, at hop 256 where there is no half-spectrum single-stream
        # entry, jdsp_stft_i16_dev, which writes 8,192 B per frame against the batch entry's 4,104.
        import ctypes as C
        from jeicyboodsp_amd import sharding
        from jeicyboodsp_amd._lib import lib as L
        lens = 2 * np.random.default_rng(10000).integers((1024 + 99 * 512) // 2, (1024 + 500 * 512) // 2, 10000)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        gen = torch.Generator(device="cuda").manual_seed(10000)
        x = (torch.randn(int(offs[-1]), device="cuda", generator=gen) * 3000.0).clamp_(-32768, 32767).to(torch.int16)
        it = max(a.iters // 4, 3)
        eng.set_option("stft.window", 1)
        for hop in (512, 256):
            counts, first = sharding.stftmask_batch_layout(offs, 1024, hop)
            total = int(first[-1])
            spec = torch.empty((total, 520), dtype=torch.complex64, device="cuda")
            what = "10,000 ragged utterances, %d frames (%d..%d each), hop %d, pitch 520" % (total, counts.min(), counts.max(), hop)
            eng.stft_half_batch(x, offs, hop=hop, pitch=520, out=spec)        # the synthesis leg's input
            if on("stft_half_batch"):
                flops = 5 * 512 * 9 + 512 * 14
                nbytes = 2 * hop + 513 * 8
                inp = "one copy: %.1f GB of PCM (from HBM), %.1f GB of spectra out" % (2e-9 * x.numel(), 8e-9 * spec.numel())
                full = torch.empty((total, 1024), dtype=torch.complex64, device="cuda")
                h, px, pf = eng._h, x.data_ptr(), full.data_ptr()
                calls = [(h, C.c_void_p(px + 2 * int(offs[u])), int(counts[u]), 1024, hop, C.c_void_p(pf + 8192 * int(first[u])))
                         for u in range(len(counts))]
                eng._use_torch_stream()

                def loop():
                    for p in calls:
                        L.jdsp_stft_i16_dev(*p)

                batch = lambda: eng.stft_half_batch(x, offs, hop=hop, pitch=520, out=spec)  # noqa: E731
                if hop == 512:
                    stream, c_what = (lambda: eng.stft_half(x, total, out=spec, pitch=520)), "one jdsp_stft_half_i16_dev, pitch 520"
                else:
                    stream, c_what = (lambda: eng.stft(x, total, 1024, hop, out=full)), \
                        "one jdsp_stft_i16_dev (all 1024 bins: 8,192 B per frame written)"
                ms_a, ms_c, ms_b = timed_alternated([batch, stream, loop], [it, it, 1], rounds=3)
                report("stft_half_batch_1024_hop%d" % hop, ms_a, total, "frames", nbytes, flops,
                       "(a) jdsp_stft_half_batch_dev, one launch: %s; %.2f x the single stream (c), %.3f of the "
                       "per-utterance loop (b)" % (what, ms_a / ms_c, ms_a / ms_b), inp=inp)
                report("stft_half_batch_1024_hop%d_per_utterance_loop" % hop, ms_b, total, "frames", 2 * hop + 8192, flops,
                       "(b) the same batch as 10,000 x jdsp_stft_i16_dev (all 1024 bins), from ctypes with precomputed "
                       "arguments: %.1f x the batch entry" % (ms_b / ms_a), inp=inp)
                report("stft_half_batch_1024_hop%d_single_stream" % hop, ms_c, total, "frames",
                       nbytes if hop == 512 else 2 * hop + 8192, flops,
                       "(c) ONE stream of the same %d frames over the same PCM: %s" % (total, c_what), inp=inp)
                del full, calls
                eng.stft_half_batch(x, offs, hop=hop, pitch=520, out=spec)    # (c) wrote other rows over it
            if on("istft_batch"):
                flops = 5 * 512 * 9 + 512 * 14
                nbytes = 513 * 8 + 2 * hop
                inp = "one copy: %.1f GB of spectra per call (from HBM), %.1f GB of PCM out" % (8e-9 * spec.numel(), 2e-9 * x.numel())
                o16 = torch.empty(x.numel(), dtype=torch.int16, device="cuda")
                ist = eng.istft(n_fft=1024, hop=hop, layout="half", synthesis_window="hann", analysis_window="hann")
                h, ps, po = ist._h, spec.data_ptr(), o16.data_ptr()
                calls = []
                for u in range(len(counts)):
                    s, f = int(offs[u]), int(counts[u])
                    calls.append(((h, C.c_void_p(ps + 8 * 520 * int(first[u])), 520, f, C.c_void_p(po + 2 * s), None),
                                  (h, C.c_void_p(po + 2 * (s + hop * f)), None)))
                eng._use_torch_stream()

                def loop():
                    for p, fl in calls:
                        L.jdsp_istft_process_dev(*p)
                        L.jdsp_istft_flush_dev(*fl)

                def stream():
                    ist.process(spec, n_frames=total, out=o16)

                ms_a, ms_c, ms_b = timed_alternated([lambda: ist.process_batch(spec, counts, offs, out=o16), stream, loop],
                                                    [it, it, 1], rounds=3)
                ist.flush()
                report("istft_batch_1024_hop%d_half" % hop, ms_a, total, "frames", nbytes, flops,
                       "(a) jdsp_istft_batch_dev, one launch: %s; %.2f x the single stream (c), %.3f of the per-utterance "
                       "loop (b)" % (what, ms_a / ms_c, ms_a / ms_b), inp=inp)
                report("istft_batch_1024_hop%d_half_per_utterance_loop" % hop, ms_b, total, "frames", nbytes, flops,
                       "(b) the same batch as 10,000 x (jdsp_istft_process_dev + jdsp_istft_flush_dev) on one handle, from "
                       "ctypes with precomputed arguments: %.1f x the batch entry" % (ms_b / ms_a), inp=inp)
                report("istft_batch_1024_hop%d_half_single_stream" % hop, ms_c, total, "frames", nbytes, flops,
                       "(c) ONE stream of the same %d frames over the same buffers, one jdsp_istft_process_dev" % total, inp=inp)
                ist.close()
                del o16, calls
            del spec
        eng.set_option("stft.window", 0)
        del x
    if on("denoise"):
        x = pcm_of(rng, B * 512)
        x[:12 * 512] = pcm_of(rng, 12 * 512, 45.0)          # the estimate latches at block 10
        t = torch.from_numpy(x).cuda()
        tr_ = rot(t)
        for mode, nm in ((0, "specsub"), (1, "wiener")):
            d = eng.denoiser(mode)
            d.set_option("blocks_per_wave", a.denoise_k)
            d.process(t)                                        # sizes the workspace

            ms = timed(lambda: d.process(tr_()), a.iters)       # steady state: one stream fed 65,536 blocks per call
            # 512 int16 in + 512 int16 out per block; forward + inverse 1024-pt real transforms
            report("denoise_" + nm, ms, B, "blocks", 2048, 2 * 5 * 512 * 9 + 2 * 512 * 14,
                   "VAD + plan + noise estimate + fused window/FFT/gain/IFFT/OLA, 65,536 blocks of 512",
                   cpu=cpu_rate(lambda: orc.denoise_stream(mode, x[:1024 * 512]), 1024))
            d.close()
        # BASELINE config 3 as worded: 512-point frames, hop 256 (two frames per wave transform), 65,536 blocks of 256
        x5 = pcm_of(rng, B * 256)
        q = (np.abs(rng.normal(0, 45, 24 * 256)) + 14.0) * np.where(np.arange(24 * 256) % 2 == 0, 1.0, -1.0)
        x5[:24 * 256] = np.rint(q).astype(np.int16)         # sign-alternating quiet start: ZCR >= 200, so the estimate latches
        t5 = torch.from_numpy(x5).cuda()
        t5r = rot(t5)
        for mode, nm in ((0, "specsub"), (1, "wiener")):
            d = eng.denoiser(mode, 512, 256)
            d.process(t5)
            ms = timed(lambda: d.process(t5r()), a.iters)
            report("denoise_" + nm + "_512pt_hop256", ms, B, "blocks", 1024, 2 * 5 * 256 * 8 + 2 * 256 * 14,
                   "BASELINE config 3 as worded: FFT_PROCESSING_SIZE 512, BLOCK_LEN 256; 65,536 blocks of 256",
                   cpu=cpu_rate(lambda: orc.denoise_stream(mode, x5[:1024 * 256], block=256), 1024))
            d.close()
    if on("denoise_batch"):
        # Batched spectral subtraction / Wiener (jdsp_denoise_batch_dev) on the stftmask_batch leg's 10,000 seeded
        # utterances (100..500 blocks of 512 each, packed), every utterance with a quiet lead of 12 blocks so that an
        # estimate latches at its block 9.  Timed three ways in this process, in alternated rounds: (a) the batch entry;
        # (b) jdsp_denoise_reset + jdsp_denoise_process_dev per utterance on one handle, from ctypes with every argument
        # computed beforehand; (c) ONE jdsp_denoise_process_dev over the same buffer as a single stream of the same
        # block count (a continuing stream: its pre-passes run in their long-stream forms, and its output differs).
        # The PCM (3 GB) is far past the 256 MiB Infinity Cache, so one copy already comes from HBM.
        import ctypes as C
        from jeicyboodsp_amd import sharding
        from jeicyboodsp_amd._lib import lib as L
        lens = 2 * np.random.default_rng(10000).integers((1024 + 99 * 512) // 2, (1024 + 500 * 512) // 2, 10000)
        counts, _ = sharding.stftmask_batch_layout(np.concatenate([[0], np.cumsum(lens)]), 1024, 512)
        sample_first, block_first, n_samples = sharding.denoise_batch_layout(counts, 512)
        total = int(block_first[-1])
        gen = torch.Generator(device="cuda").manual_seed(10000)
        sigma = torch.full((total,), 3000.0, device="cuda")
        lead = torch.from_numpy((block_first[:-1, None] + np.arange(12)[None, :]).ravel()).cuda()
        sigma[lead] = 45.0
        x = torch.empty(n_samples, dtype=torch.int16, device="cuda")
        for lo in range(0, total, 1 << 18):                     # in slabs: the float32 draft of 1.5 G samples is 6 GB
            hi = min(lo + (1 << 18), total)
            draft = torch.randn((hi - lo, 512), device="cuda", generator=gen) * sigma[lo:hi, None]
            x[lo * 512:hi * 512] = draft.round_().clamp_(-32768, 32767).to(torch.int16).view(-1)
        del draft, sigma, lead
        o16 = torch.empty(n_samples, dtype=torch.int16, device="cuda")
        it = max(a.iters // 4, 3)
        what = "10,000 ragged utterances, %d blocks (%d..%d each), 12 quiet blocks in front of each" % (total, counts.min(), counts.max())
        inp = "one copy: %.1f GB of PCM per call (from HBM)" % (2e-9 * n_samples)
        flops = 2 * 5 * 512 * 9 + 2 * 512 * 14
        for mode, nm in ((0, "specsub"), (1, "wiener")):
            d_a, d_b, d_c = eng.denoiser(mode), eng.denoiser(mode), eng.denoiser(mode)
            d_a.reserve_batch(total, len(counts))
            eng._ck(L.jdsp_denoise_reserve(d_b._h, int(counts.max())))
            eng._ck(L.jdsp_denoise_reserve(d_c._h, total))
            px, po = x.data_ptr(), o16.data_ptr()
            calls = [(d_b._h, C.c_void_p(px + 2 * int(sample_first[u])), int(counts[u]),
                      C.c_void_p(po + 2 * int(sample_first[u])), None, None) for u in range(len(counts))]
            stream_args = (d_c._h, C.c_void_p(px), total, C.c_void_p(po), None, None)
            eng._use_torch_stream()

            def loop():
                for p in calls:
                    L.jdsp_denoise_reset(p[0])
                    L.jdsp_denoise_process_dev(*p)

            batch = lambda: d_a.process_batch(x, counts, sample_first, out=o16)  # noqa: E731
            stream = lambda: L.jdsp_denoise_process_dev(*stream_args)  # noqa: E731
            ms_a, ms_c, ms_b = timed_alternated([batch, stream, loop], [it, it, 1], rounds=3)
            n_redo = d_a.frames_recomputed()
            report("denoise_batch_" + nm, ms_a, total, "blocks", 2048, flops,
                   "(a) jdsp_denoise_batch_dev: %s; %.2f x the single stream (c), %.3f of the per-utterance loop (b); "
                   "%d frames through the FP64 pass" % (what, ms_a / ms_c, ms_a / ms_b, n_redo), inp=inp)
            report("denoise_batch_" + nm + "_per_utterance_loop", ms_b, total, "blocks", 2048, flops,
                   "(b) the same batch as 10,000 x (jdsp_denoise_reset + jdsp_denoise_process_dev) on one handle, from "
                   "ctypes with precomputed arguments: %.1f x the batch entry" % (ms_b / ms_a), inp=inp)
            report("denoise_batch_" + nm + "_single_stream", ms_c, total, "blocks", 2048, flops,
                   "(c) ONE continuing stream of the same %d blocks over the same buffer, one jdsp_denoise_process_dev" % total,
                   inp=inp)
            for d in (d_a, d_b, d_c):
                d.close()
        del x, o16
    if on("mvdrn_batch"):
        # Batched n-microphone MVDR (jdsp_mvdrn_batch_dev): 8 microphones, loading 1e-3, 2,000 seeded utterances of
        # 20..100 blocks of 512, packed, every utterance with a quiet lead of 6 blocks (5 estimation frames).  Timed three
        # ways in this process, in alternated rounds: (a) the batch entry; (b) jdsp_mvdrn_reset + jdsp_mvdrn_process_dev
        # per utterance on one handle, from ctypes with every argument computed beforehand, over the first 200
        # utterances and scaled by 10; (c) ONE jdsp_mvdrn_process_dev over the same planes as a single stream of the
        # same block count (a continuing stream: its output differs).  The PCM (about 1 GB over the eight planes) is far
        # past the 256 MiB Infinity Cache, so one copy already comes from HBM.
        import ctypes as C
        from jeicyboodsp_amd import sharding
        from jeicyboodsp_amd._lib import lib as L
        n_mics, n_utts, part = 8, 2000, 200
        counts = np.random.default_rng(2000).integers(20, 101, n_utts).astype(np.int64)
        sample_first, block_first, n_samples = sharding.denoise_batch_layout(counts, 512)
        total = int(block_first[-1])
        gen = torch.Generator(device="cuda").manual_seed(2000)
        sigma = torch.full((total,), 3000.0, device="cuda")
        sigma[torch.from_numpy((block_first[:-1, None] + np.arange(6)[None, :]).ravel()).cuda()] = 30.0
        x = torch.empty((n_mics, n_samples), dtype=torch.int16, device="cuda")
        for m in range(n_mics):
            draft = torch.randn((total, 512), device="cuda", generator=gen) * sigma[:, None]
            x[m] = draft.round_().clamp_(-32768, 32767).to(torch.int16).view(-1)
        del draft, sigma
        o16 = torch.empty(n_samples, dtype=torch.int16, device="cuda")
        m_a, m_b, m_c = (eng.mvdr_multi(n_mics, None, 1e-3) for _ in range(3))
        m_a.reserve_batch(total, n_utts)
        px, po = x.data_ptr(), o16.data_ptr()
        calls = [(m_b._h, C.c_void_p(px + 2 * int(sample_first[u])), n_samples, int(counts[u]),
                  C.c_void_p(po + 2 * int(sample_first[u])), None, None) for u in range(part)]
        stream_args = (m_c._h, C.c_void_p(px), n_samples, total, C.c_void_p(po), None, None)
        eng._use_torch_stream()

        def loop():
            for p in calls:
                L.jdsp_mvdrn_reset(p[0])
                L.jdsp_mvdrn_process_dev(*p)

        def stream():
            L.jdsp_mvdrn_reset(m_c._h)
            L.jdsp_mvdrn_process_dev(*stream_args)

        batch = lambda: m_a.process_batch(x, counts, sample_first, out=o16)  # noqa: E731
        assert L.jdsp_mvdrn_process_dev(*calls[0]) == 0 and L.jdsp_mvdrn_process_dev(*stream_args) == 0
        it = 2 * a.iters                                        # a window of about 0.1 s for (a) and (c)
        ms_a, ms_c, ms_b = timed_alternated([batch, stream, loop], [it, it, 4], rounds=5)
        ms_b *= n_utts / part
        what = "%d ragged utterances, %d blocks (%d..%d each), 8 microphones, 6 quiet blocks in front of each" % (
            n_utts, total, counts.min(), counts.max())
        inp = "one copy: %.2f GB of PCM per call (from HBM)" % (2e-9 * n_samples * n_mics)
        nbytes, flops = 8 * 1024 + 1024, 9 * 5 * 512 * 9 + 9 * 512 * 14 + 1024 * 8 * 8
        report("mvdrn_batch", ms_a, total, "blocks", nbytes, flops,
               "(a) jdsp_mvdrn_batch_dev: %s; %.2f x the single stream (c), %.4f of the per-utterance loop (b)"
               % (what, ms_a / ms_c, ms_a / ms_b), inp=inp)
        report("mvdrn_batch_per_utterance_loop", ms_b, total, "blocks", nbytes, flops,
               "(b) the same batch as %d x (jdsp_mvdrn_reset + jdsp_mvdrn_process_dev) on one handle, from ctypes with "
               "precomputed arguments: measured over the first %d utterances and scaled by %d; %.1f x the batch entry"
               % (n_utts, part, n_utts // part, ms_b / ms_a), inp=inp)
        report("mvdrn_batch_single_stream", ms_c, total, "blocks", nbytes, flops,
               "(c) ONE fresh stream of the same %d blocks over the same planes, jdsp_mvdrn_reset + one "
               "jdsp_mvdrn_process_dev" % total, inp=inp)
        for m in (m_a, m_b, m_c):
            m.close()
        del x, o16
    if on("reverb_batch"):
        # Batched reverberation (jdsp_reverb_batch_dev): 2,000 seeded utterances of 50..300 blocks of 512 (even counts: the
        # convolver's block is 1024), packed, each with its own response out of a bank of 256 x 7,169 taps, gains 1.
        # Timed three ways in this process, in alternated rounds, every C entry called through ctypes with its arguments
        # computed beforehand: (a) the batch entry; (b) 256 jdsp_fastconv handles (n_fft 8192, partitioned), one per
        # response, jdsp_fastconv_reset + jdsp_fastconv_process_dev per utterance on its response's handle, over the
        # first 200 utterances and scaled by 10 -- each call emits 7 blocks of 1024 fewer than it is fed (the
        # reference's silent head), so (b) does a little less; (c) ONE jdsp_fastconv stream of the same total block
        # count with one response.  The PCM rotates over 3 copies (one copy is already past the 256 MiB Infinity Cache).
        import ctypes as C
        from jeicyboodsp_amd import sharding
        from jeicyboodsp_amd._lib import lib as L
        n_utts, part, n_irs, n_taps = 2000, 200, 256, 7169
        rs = np.random.default_rng(2900)
        counts = 2 * rs.integers(25, 151, n_utts).astype(np.int64)
        sample_first, block_first, n_samples = sharding.denoise_batch_layout(counts, 512)
        total = int(block_first[-1])
        taps = rs.normal(size=(n_irs, n_taps)) * np.exp(-np.arange(n_taps) / 1500.0) * 0.05
        ir_h = rs.integers(0, n_irs, n_utts).astype(np.int32)
        gen = torch.Generator(device="cuda").manual_seed(2900)
        x = (torch.randn(n_samples, device="cuda", generator=gen) * 3000.0).round_().clamp_(-32768, 32767).to(torch.int16)
        ins = [x] if a.warm else [x, x.clone(), x.clone()]
        o16 = torch.empty(n_samples, dtype=torch.int16, device="cuda")
        d_first, d_bf = torch.from_numpy(sample_first).cuda(), torch.from_numpy(block_first).cuda()
        d_ir = torch.from_numpy(ir_h).cuda()
        rv = eng.reverb(taps)
        rv.reserve_batch(total, n_utts)
        used = sorted(set(ir_h[:part].tolist()))
        convs = {i: eng.fastconv(taps[i], 8192) for i in range(n_irs)}
        one = eng.fastconv(taps[0], 8192)
        for c in convs.values():
            assert L.jdsp_fastconv_reserve(c._h, int(counts[:part].max()) // 2) == 0
        assert L.jdsp_fastconv_reserve(one._h, total // 2) == 0
        po = o16.data_ptr()
        args_a = [(rv._h, C.c_void_p(t.data_ptr()), C.c_void_p(d_first.data_ptr()), C.c_void_p(d_bf.data_ptr()),
                   C.c_void_p(d_ir.data_ptr()), None, n_utts, total, C.c_void_p(po), None) for t in ins]
        calls = [[(convs[int(ir_h[u])]._h, C.c_void_p(t.data_ptr() + 2 * int(sample_first[u])), int(counts[u]) // 2,
                   C.c_void_p(po + 2 * int(sample_first[u])), None, None) for u in range(part)] for t in ins]
        args_c = [(one._h, C.c_void_p(t.data_ptr()), total // 2, C.c_void_p(po), None, None) for t in ins]
        turn = [0, 0, 0]
        eng._use_torch_stream()

        def batch():
            turn[0] += 1
            L.jdsp_reverb_batch_dev(*args_a[turn[0] % len(ins)])

        def loop():
            turn[1] += 1
            for p in calls[turn[1] % len(ins)]:
                L.jdsp_fastconv_reset(p[0])
                L.jdsp_fastconv_process_dev(*p)

        def stream():
            turn[2] += 1
            L.jdsp_fastconv_reset(one._h)
            L.jdsp_fastconv_process_dev(*args_c[turn[2] % len(ins)])

        assert L.jdsp_reverb_batch_dev(*args_a[0]) == 0 and L.jdsp_fastconv_process_dev(*calls[0][0]) == 0
        assert L.jdsp_fastconv_process_dev(*args_c[0]) == 0
        ms_a, ms_c, ms_b = timed_alternated([batch, stream, loop], [a.iters, a.iters, 2], rounds=5)
        ms_b *= n_utts / part
        what = "%d ragged utterances, %d blocks of 512 (%d..%d each), %d responses x %d taps (P = %d), gains 1" % (
            n_utts, total, counts.min(), counts.max(), n_irs, n_taps, rv.n_part)
        inp = "rotated over %d copies of %.0f MB (from HBM)" % (len(ins), 2e-6 * n_samples)
        ws = 4160 * total + 8 * (n_utts + 1)
        nbytes = 1024 + 1024
        flops = 2 * (5 * 512 * 9 + 512 * 14) + 8 * 513 * rv.n_part
        report("reverb_batch", ms_a, total, "blocks", nbytes, flops,
               "(a) jdsp_reverb_batch_dev: %s; workspace %.2f GB, bank %.1f MB; %.2f x the single stream (c), %.4f of the "
               "per-utterance loop (b)" % (what, 1e-9 * ws, 1e-6 * 4160 * rv.n_part * n_irs, ms_a / ms_c, ms_a / ms_b), inp=inp)
        report("reverb_batch_per_utterance_loop", ms_b, total, "blocks", nbytes, flops,
               "(b) the same batch as %d x (jdsp_fastconv_reset + jdsp_fastconv_process_dev), one jdsp_fastconv handle per "
               "response, from ctypes with precomputed arguments: measured over the first %d utterances (%d of the 256 handles) and "
               "scaled by %d; every call emits 7 blocks of 1024 fewer than it is fed; %.1f x the batch entry"
               % (n_utts, part, len(used), n_utts // part, ms_b / ms_a), inp=inp)
        report("reverb_batch_single_stream", ms_c, total, "blocks", nbytes, flops,
               "(c) ONE jdsp_fastconv stream of the same %d blocks of 512 with one response, jdsp_fastconv_reset + one "
               "jdsp_fastconv_process_dev" % total, inp=inp)
        rv.close()
        one.close()
        for c in convs.values():
            c.close()
        del x, ins, o16
    if on("reverb_streams"):
        # Live reverberation streams (jdsp_reverb_streams_dev): 2,000 live streams warmed with P blocks each, a bank of
        # 256 responses x 7,169 taps (P = 15), stream s on response s mod 256, `per` NEW blocks per delivery, int16 out.
        # Timed three ways in this process, in alternated rounds, every C entry called through ctypes with its arguments
        # computed beforehand: (a) the live entry, every call a further delivery to all streams; (b) today's route,
        # jdsp_reverb_batch_dev over 2,000 utterances of P + per blocks (the history presented again; the repacking
        # copy is not counted), of which per are kept; (c) the stateless floor, jdsp_reverb_batch_dev over the same
        # per-block chunks as fresh utterances (another result).  per = 4 is the figure, 1 and 32 are recorded beside
        # it; at per = 4, (d) one jdsp_fastconv handle (n_fft 8192, blocks of 1024) per stream in a loop of
        # jdsp_fastconv_process_dev, over the first 100 streams and scaled by 20.  The PCM rotates over 6 copies; what
        # (a) moves on top is each stream's ring, which no cache holds at 116 MB.
        import ctypes as C
        from jeicyboodsp_amd import sharding
        from jeicyboodsp_amd._lib import lib as L
        n_streams, n_irs, n_taps, part = 2000, 256, 7169, 100
        rs = np.random.default_rng(3000)
        taps = rs.normal(size=(n_irs, n_taps)) * np.exp(-np.arange(n_taps) / 1500.0) * 0.05
        rv = eng.reverb(taps)
        P = rv.n_part
        ids_h = np.arange(n_streams, dtype=np.int64)
        ir_h = (ids_h % n_irs).astype(np.int32)
        d_ids, d_ir = torch.from_numpy(ids_h).cuda(), torch.from_numpy(ir_h).cuda()
        gen = torch.Generator(device="cuda").manual_seed(3000)
        vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731

        def noise(n):
            return (torch.randn(n, device="cuda", generator=gen) * 3000.0).round_().clamp_(-32768, 32767).to(torch.int16)

        eng._use_torch_stream()
        for per in (4, 1, 32):
            lay = {}
            for key, nb in (("a", per), ("b", P + per), ("w", P)):
                sf, bf, ns = sharding.denoise_batch_layout(np.full(n_streams, nb, np.int64), 512)
                lay[key] = (torch.from_numpy(sf).cuda(), torch.from_numpy(bf).cuda(), ns, int(bf[-1]))
            xa, xb = rot(noise(lay["a"][2])), rot(noise(lay["b"][2]))
            o16 = torch.empty(lay["b"][2], dtype=torch.int16, device="cuda")
            rv.open_streams(n_streams, max(lay["a"][3], lay["w"][3]))
            rv.reserve_batch(lay["b"][3], n_streams)
            warm = noise(lay["w"][2])
            assert L.jdsp_reverb_streams_dev(rv._h, vp(warm), vp(d_ids), vp(lay["w"][0]), vp(lay["w"][1]), vp(d_ir), None,
                                             n_streams, lay["w"][3], None, None) == 0

            def live():
                L.jdsp_reverb_streams_dev(rv._h, vp(xa()), vp(d_ids), vp(lay["a"][0]), vp(lay["a"][1]), vp(d_ir), None,
                                          n_streams, lay["a"][3], vp(o16), None)

            def again():
                L.jdsp_reverb_batch_dev(rv._h, vp(xb()), vp(lay["b"][0]), vp(lay["b"][1]), vp(d_ir), None, n_streams,
                                        lay["b"][3], vp(o16), None)

            def fresh():
                L.jdsp_reverb_batch_dev(rv._h, vp(xa()), vp(lay["a"][0]), vp(lay["a"][1]), vp(d_ir), None, n_streams,
                                        lay["a"][3], vp(o16), None)

            it = max(25 * a.iters, 100)                         # a call is 0.05 to 0.6 ms: windows of tens of ms and more
            fns, iters = [live, again, fresh], [it, it, it]
            if per == 4:
                convs = [eng.fastconv(taps[int(ir_h[s])], 8192) for s in range(part)]
                for c in convs:
                    assert c.block == 1024 and L.jdsp_fastconv_reserve(c._h, per // 2) == 0
                sf_h = np.arange(n_streams, dtype=np.int64) * per * 512

                def loop():
                    px, po = xa().data_ptr(), o16.data_ptr()
                    for s, c in enumerate(convs):
                        off = 2 * int(sf_h[s])
                        L.jdsp_fastconv_process_dev(c._h, C.c_void_p(px + off), per // 2, C.c_void_p(po + off), None, None)

                for _ in range(P):                              # past the convolver's silent head: every call emits
                    loop()
                fns.append(loop)
                iters.append(2)
            ms = timed_alternated(fns, iters, rounds=5)
            ms_a, ms_b, ms_c = ms[:3]
            seen = rv.streams_state([0, n_streams - 1])[0]
            assert seen.min() > P + per * a.iters
            total = lay["a"][3]
            what = "%d live streams x %d new blocks per delivery, %d responses x %d taps (P = %d), gains 1" % (
                n_streams, per, n_irs, n_taps, P)
            inp = "rotated over 6 copies: %.1f MB of PCM per call of (a) and (c), %.1f MB of (b)" % (
                2e-6 * lay["a"][2], 2e-6 * lay["b"][2])
            state = 4160 * (P - 1) + 1032
            nbytes = 1024 + 1024
            flops = 2 * (5 * 512 * 9 + 512 * 14) + 8 * 513 * P
            tag = "" if per == 4 else "_%dblocks" % per
            report("reverb_streams" + tag, ms_a, total, "blocks", nbytes, flops,
                   "(a) jdsp_reverb_streams_dev: %s; %.3f of today's route (b), %.2f x the stateless floor (c); state %d "
                   "bytes per stream, %.1f MB in all" % (what, ms_a / ms_b, ms_a / ms_c, state, 1e-6 * state * n_streams), inp=inp)
            report("reverb_streams_history_again" + tag, ms_b, total, "blocks", nbytes, flops,
                   "(b) jdsp_reverb_batch_dev over %d utterances of P + %d = %d blocks, the history presented again, %d "
                   "kept: %.2f x the transforms and accumulations; %.2f x the live entry"
                   % (n_streams, per, P + per, per, (P + per) / per, ms_b / ms_a), inp=inp)
            report("reverb_streams_fresh_batch" + tag, ms_c, total, "blocks", nbytes, flops,
                   "(c) jdsp_reverb_batch_dev over the same %d chunks of %d blocks as fresh utterances (no carried state: "
                   "another result)" % (n_streams, per), inp=inp)
            if per == 4:
                ms_d = ms[3] * n_streams / part
                report("reverb_streams_fastconv_loop", ms_d, total, "blocks", nbytes, flops,
                       "(d) the same delivery as %d x jdsp_fastconv_process_dev (n_fft 8192, 2 blocks of 1024), one handle per "
                       "stream, from ctypes: measured over the first %d streams and scaled by %d; %.1f x the live entry"
                       % (n_streams, part, n_streams // part, ms_d / ms_a), inp=inp)
                for c in convs:
                    c.close()
            del xa, xb, o16, warm
        rv.close()
    if on("mvdrn_streams"):
        # Live n-microphone MVDR streams (jdsp_mvdrn_streams_dev): 1,000 live streams x 4 blocks per delivery, 8
        # microphones, loading 1e-3, the first two blocks of every chunk quiet (one estimation frame per chunk and
        # delivery).  Timed three ways in this process, in alternated rounds: (a) the live entry, every call a further
        # delivery to all streams; (b) one jdsp_mvdrn handle per stream and jdsp_mvdrn_process_dev per delivery, from
        # ctypes with the handles made beforehand, over the first 100 streams and scaled by 10; (c)
        # jdsp_mvdrn_batch_dev over the same chunks as fresh utterances, the stateless floor.  The PCM (33 MB over the
        # eight planes) rotates over 6 copies; (a) moves the covariances on top, which no cache holds.
        import ctypes as C
        from jeicyboodsp_amd import sharding
        from jeicyboodsp_amd._lib import lib as L
        n_mics, n_streams, per, part = 8, 1000, 4, 100
        counts = np.full(n_streams, per, np.int64)
        sample_first, block_first, n_samples = sharding.denoise_batch_layout(counts, 512)
        total = int(block_first[-1])
        gen = torch.Generator(device="cuda").manual_seed(1000)
        sigma = torch.full((total,), 3000.0, device="cuda")
        sigma[torch.from_numpy((block_first[:-1, None] + np.arange(2)[None, :]).ravel()).cuda()] = 30.0
        x = torch.empty((n_mics, n_samples), dtype=torch.int16, device="cuda")
        for m in range(n_mics):
            draft = torch.randn((total, 512), device="cuda", generator=gen) * sigma[:, None]
            x[m] = draft.round_().clamp_(-32768, 32767).to(torch.int16).view(-1)
        del draft, sigma
        xr = rot(x)
        o16 = torch.empty(n_samples, dtype=torch.int16, device="cuda")
        m_a, m_c = eng.mvdr_multi(n_mics, None, 1e-3), eng.mvdr_multi(n_mics, None, 1e-3)
        m_a.open_streams(n_streams, total)
        m_c.reserve_batch(total, n_streams)
        singles = [eng.mvdr_multi(n_mics, None, 1e-3) for _ in range(part)]
        ids = np.arange(n_streams, dtype=np.int64)
        po = o16.data_ptr()
        eng._use_torch_stream()

        def loop():
            px = xr().data_ptr()
            for u, h in enumerate(singles):
                off = 2 * int(sample_first[u])
                L.jdsp_mvdrn_process_dev(h._h, C.c_void_p(px + off), n_samples, per, C.c_void_p(po + off), None, None)

        live = lambda: m_a.process_streams(xr(), ids, counts, sample_first, out=o16)  # noqa: E731
        batch = lambda: m_c.process_batch(xr(), counts, sample_first, out=o16)  # noqa: E731
        loop()                                                  # every handle's first call: its workspace, no emission
        ms_a, ms_c, ms_b = timed_alternated([live, batch, loop], [a.iters, a.iters, 4], rounds=5)
        ms_b *= n_streams / part
        assert m_a.streams_state([0, n_streams - 1]).min() > per * a.iters
        state_bytes = 2 * 513 * 64 * 16                         # a stream's covariance, read and written per delivery
        what = "%d live streams x %d blocks per delivery, 8 microphones, one estimation frame per chunk" % (n_streams, per)
        inp = "rotated over 6 copies: %.1f MB of PCM per call" % (2e-6 * n_samples * n_mics)
        nbytes, flops = 8 * 1024 + 1024, 9 * 5 * 512 * 9 + 9 * 512 * 14 + 1024 * 8 * 8
        report("mvdrn_streams", ms_a, total, "blocks", nbytes + state_bytes // per, flops,
               "(a) jdsp_mvdrn_streams_dev: %s; %.2f x the batch of fresh utterances (c), %.4f of the per-stream loop (b); "
               "on top of (c) it moves each stream's covariance in and out, %.2f GB per call (%d bytes per block)"
               % (what, ms_a / ms_c, ms_a / ms_b, 1e-9 * state_bytes * n_streams, state_bytes // per), inp=inp)
        report("mvdrn_streams_per_stream_loop", ms_b, total, "blocks", nbytes, flops,
               "(b) the same delivery as %d x jdsp_mvdrn_process_dev, one handle per stream, from ctypes: measured over "
               "the first %d streams and scaled by %d; %.1f x the live entry" % (n_streams, part, n_streams // part, ms_b / ms_a),
               inp=inp)
        report("mvdrn_streams_fresh_batch", ms_c, total, "blocks", nbytes, flops,
               "(c) jdsp_mvdrn_batch_dev over the same %d chunks as fresh utterances (no carried state: another result)"
               % n_streams, inp=inp)
        for m in [m_a, m_c] + singles:
            m.close()
        del x, xr, o16
    if on("stftmask_streams") or on("istft_streams"):
        # Live streams (jdsp_stftmask_streams_dev, jdsp_istft_streams_dev): 10,000 live streams, every call brings each
        # of them a chunk of 4 frames, hop 256 and 512, real mask / half layout (pitch 513).  Timed three ways in this
        # process, in alternated rounds, every C entry called through ctypes with its arguments computed beforehand:
        # (a) the streams entry, the transform launch plus the commit launch; (b) one single-stream handle per stream in
        # a loop of _process_dev -- over the first 1,000 streams, the figure scaled by 10 --; (c) the stateless _batch_dev
        # entry over the same chunks as utterances, the yardstick.  The inputs rotate over 6 copies (0.7-1.0 GB in all,
        # past the 256 MiB Infinity Cache); the calls of (a) follow each other as the calls of a service do, every
        # stream carrying its tail on.  Bytes per chunk come from the shapes: against (c), (a) reads and writes a tail
        # of 4 (n - hop) bytes and does not write (c)'s emitted tail of 2 (n - hop).
        import ctypes as C
        from jeicyboodsp_amd import sharding
        from jeicyboodsp_amd._lib import lib as L
        S, F, n, n_loop, pitch = 10000, 4, 1024, 1000, 513
        gen = torch.Generator(device="cuda").manual_seed(18)
        ids = torch.from_numpy(np.random.default_rng(18).permutation(S).astype(np.int64)).cuda()
        vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731
        it, rounds = max(100 * a.iters, 200), 3
        for kind in ("stftmask", "istft"):
            if not on(kind + "_streams"):
                continue
            for hop in (256, 512):
                counts = np.full(S, F, np.int64)
                sf_a, ff, n_a = sharding.stream_chunks_layout(counts, n, hop, kind == "stftmask")
                d_ff = torch.from_numpy(ff).cuda()
                d_sf_a = torch.from_numpy(sf_a).cuda()
                total = S * F
                tail = 4 * (n - hop)
                span = hop * (F - 1) + n
                if kind == "stftmask":
                    sm = eng.stft_mask(n_fft=n, hop=hop, analysis_window="hann", synthesis_window="hann", normalise=1)
                    sm.open_streams(S)
                    ins = [((torch.randn(n_a, device="cuda", generator=gen) * 3000.0).clamp_(-32768, 32767).to(torch.int16),
                            torch.rand((total, pitch), dtype=torch.float32, device="cuda", generator=gen) * 1.5)
                           for _ in range(1 if a.warm else 6)]
                    o16 = torch.empty(n_a, dtype=torch.int16, device="cuda")
                    args_a = [(sm._h, vp(x), vp(m), pitch, vp(ids), vp(d_sf_a), vp(d_ff), S, total, vp(o16), None) for x, m in ins]
                    args_c = [(sm._h, vp(x), vp(m), pitch, vp(d_sf_a), vp(d_ff), S, total, vp(o16), None) for x, m in ins]
                    ent_a, ent_c, ent_b = L.jdsp_stftmask_streams_dev, L.jdsp_stftmask_batch_dev, L.jdsp_stftmask_process_dev
                    singles = [eng.stft_mask(n_fft=n, hop=hop, analysis_window="hann", synthesis_window="hann", normalise=1)
                               for _ in range(n_loop)]
                    x0, m0 = ins[0]
                    args_b = [(h._h, vp(x0, 2 * int(sf_a[u])), vp(m0, 4 * pitch * F * u), pitch, F, vp(o16, 2 * int(sf_a[u])), None)
                              for u, h in enumerate(singles)]
                    common = 2 * span + F * pitch * 4
                    bytes_a, bytes_c = common + 2 * hop * F + 2 * tail, common + 2 * span
                    what = "real mask"
                else:
                    sm = eng.istft(n_fft=n, hop=hop, layout="half", synthesis_window="hann", analysis_window="hann")
                    sm.open_streams(S)
                    ins = [torch.randn((total, pitch), dtype=torch.complex64, device="cuda", generator=gen) * 3000.0 * np.sqrt(n)
                           for _ in range(1 if a.warm else 6)]
                    sf_c, _ = sharding.istft_batch_layout(counts, n, hop)
                    d_sf_c = torch.from_numpy(np.ascontiguousarray(sf_c[:-1])).cuda()
                    o16 = torch.empty(int(sf_c[-1]), dtype=torch.int16, device="cuda")
                    args_a = [(sm._h, vp(s), pitch, vp(ids), vp(d_sf_a), vp(d_ff), S, total, vp(o16), None) for s in ins]
                    args_c = [(sm._h, vp(s), pitch, vp(d_sf_c), vp(d_ff), S, total, vp(o16), None) for s in ins]
                    ent_a, ent_c, ent_b = L.jdsp_istft_streams_dev, L.jdsp_istft_batch_dev, L.jdsp_istft_process_dev
                    singles = [eng.istft(n_fft=n, hop=hop, layout="half", synthesis_window="hann", analysis_window="hann")
                               for _ in range(n_loop)]
                    args_b = [(h._h, vp(ins[0], 8 * pitch * F * u), pitch, F, vp(o16, 2 * int(sf_a[u])), None)
                              for u, h in enumerate(singles)]
                    common = F * pitch * 8
                    bytes_a, bytes_c = common + 2 * hop * F + 2 * tail, common + 2 * span
                    what = "half layout"
                eng._use_torch_stream()
                turn = [0]

                def call_a():
                    turn[0] += 1
                    ent_a(*args_a[turn[0] % len(args_a)])

                def call_c():
                    turn[0] += 1
                    ent_c(*args_c[turn[0] % len(args_c)])

                def loop():
                    for p in args_b:
                        ent_b(*p)

                assert ent_a(*args_a[0]) == 0 and ent_c(*args_c[0]) == 0 and ent_b(*args_b[0]) == 0
                ms_a, ms_c, ms_b = timed_alternated([call_a, call_c, loop], [it, it, 1], rounds=rounds)
                ms_b *= S / n_loop
                flops = (2 if kind == "stftmask" else 1) * (5 * 512 * 9 + 512 * 14)
                inp = "rotated over %d copies of %.0f MB (from HBM)" % (len(ins), 1e-6 * S * common)
                shape = "10,000 live streams x 4 frames per call, hop %d, %s" % (hop, what)
                report("%s_streams_1024_hop%d" % (kind, hop), ms_a, total, "frames", bytes_a / F, flops,
                       "(a) jdsp_%s_streams_dev, the transform launch and the commit launch: %s; (a)/(c) = %.3f against a "
                       "byte ratio of %.3f (%d against %d bytes per chunk); %.4f of the per-stream loop (b); %d calls per "
                       "round, %d rounds" % (kind, shape, ms_a / ms_c, bytes_a / bytes_c, bytes_a, bytes_c, ms_a / ms_b, it, rounds),
                       inp=inp)
                report("%s_streams_1024_hop%d_per_stream_loop" % (kind, hop), ms_b, total, "frames", bytes_a / F, flops,
                       "(b) one single-stream handle per stream, a loop of jdsp_%s_process_dev from ctypes with precomputed "
                       "arguments: measured over %d streams and scaled by %d; %.1f x the streams entry"
                       % (kind, n_loop, S // n_loop, ms_b / ms_a), inp=inp)
                report("%s_streams_1024_hop%d_stateless_batch" % (kind, hop), ms_c, total, "frames", bytes_c / F, flops,
                       "(c) the yardstick: jdsp_%s_batch_dev over the same chunks as utterances, nothing carried" % kind, inp=inp)
                for h in singles:
                    h.close()
                sm.close()
                del ins, o16, args_a, args_b, args_c, singles
    if on("denoise_streams"):
        # Live denoise streams (jdsp_denoise_streams_dev): 10,000 live streams, every call brings each of them a chunk
        # of 4 blocks; a chunk is quiet (sigma 45) or loud (sigma 3000) at even odds, so runs of quiet blocks build up,
        # latch and break across the calls.  Timed three ways in this process, in alternated rounds, every C entry called
        # through ctypes with its arguments computed beforehand: (a) the streams entry -- VAD, noise pass, run kernel,
        # FP64 pass (spectral subtraction) and commit --; (b) one jdsp_denoise handle per stream in a loop of
        # _process_dev, over the first 1,000 streams and scaled by 10; (c) the stateless jdsp_denoise_batch_dev over the
        # same chunks as utterances: other arithmetic at the boundaries, the same work, the yardstick.  The inputs rotate
        # over 8 copies of 41 MB (328 MB, past the 256 MiB Infinity Cache).  Bytes per chunk come from the shapes:
        # both read the chunk's 4 blocks; (c) writes 2 blocks, (a) writes 4 and reads and writes the stream's state.
        import ctypes as C
        from jeicyboodsp_amd import sharding
        from jeicyboodsp_amd._lib import lib as L
        S, F, n_loop = 10000, 4, 1000
        gen = torch.Generator(device="cuda").manual_seed(19)
        ids = torch.from_numpy(np.random.default_rng(19).permutation(S).astype(np.int64)).cuda()
        vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731
        it, rounds = max(25 * a.iters, 100), 3
        counts = np.full(S, F, np.int64)
        sf, bf, n_samples = sharding.denoise_batch_layout(counts, 512)
        d_sf, d_bf = torch.from_numpy(sf).cuda(), torch.from_numpy(bf).cuda()
        total = S * F
        ins = []
        for _ in range(1 if a.warm else 8):
            sigma = torch.where(torch.rand(S, device="cuda", generator=gen) < 0.5, 45.0, 3000.0)
            draft = torch.randn((S, F * 512), device="cuda", generator=gen) * sigma[:, None]
            ins.append(draft.round_().clamp_(-32768, 32767).to(torch.int16).view(-1))
        del draft, sigma
        o16 = torch.empty(n_samples, dtype=torch.int16, device="cuda")
        block = 1024                                            # bytes of a block of int16
        # the state a chunk reads and writes: one previous block in, two out; the overlap in and out (float32); the
        # running average in and out; the estimate in force in; the words
        state = block + 2 * block + 2 * 2048 + 2 * 2560 + 4096 + 28
        bytes_a, bytes_c = F * block + F * block + state, F * block + (F - 2) * block
        flops = 2 * 5 * 512 * 9 + 2 * 512 * 14
        for mode, nm in ((0, "specsub"), (1, "wiener")):
            d_a, d_c = eng.denoiser(mode), eng.denoiser(mode)
            d_a.open_streams(S, total)
            d_c.reserve_batch(total, S)
            singles = [eng.denoiser(mode) for _ in range(n_loop)]
            for h in singles:
                eng._ck(L.jdsp_denoise_reserve(h._h, F))
            args_a = [(d_a._h, vp(x), vp(ids), vp(d_sf), vp(d_bf), S, total, vp(o16), None, None, None) for x in ins]
            args_c = [(d_c._h, vp(x), vp(d_sf), vp(d_bf), S, total, vp(o16), None, None, None) for x in ins]
            args_b = [(h._h, vp(ins[0], 2 * int(sf[u])), F, vp(o16, 2 * int(sf[u])), None, None) for u, h in enumerate(singles)]
            eng._use_torch_stream()
            turn = [0]

            def call_a():
                turn[0] += 1
                L.jdsp_denoise_streams_dev(*args_a[turn[0] % len(args_a)])

            def call_c():
                turn[0] += 1
                L.jdsp_denoise_batch_dev(*args_c[turn[0] % len(args_c)])

            def loop():
                for p in args_b:
                    L.jdsp_denoise_process_dev(*p)

            assert L.jdsp_denoise_streams_dev(*args_a[0]) == 0 and L.jdsp_denoise_batch_dev(*args_c[0]) == 0
            assert L.jdsp_denoise_process_dev(*args_b[0]) == 0
            ms_a, ms_c, ms_b = timed_alternated([call_a, call_c, loop], [it, it, 1], rounds=rounds)
            ms_b *= S / n_loop
            n_redo = d_a.frames_recomputed()
            inp = "rotated over %d copies of %.0f MB (from HBM)" % (len(ins), 2e-6 * n_samples)
            shape = "10,000 live streams x 4 blocks per call, chunks quiet or loud at even odds"
            report("denoise_streams_" + nm, ms_a, total, "blocks", bytes_a / F, flops,
                   "(a) jdsp_denoise_streams_dev: %s; (a)/(c) = %.3f against a byte ratio of %.3f (%d against %d bytes per "
                   "chunk, %d of them state); %.4f of the per-stream loop (b); %d frames through the FP64 pass in the last "
                   "call; %d calls per round, %d rounds"
                   % (shape, ms_a / ms_c, bytes_a / bytes_c, bytes_a, bytes_c, state, ms_a / ms_b, n_redo, it, rounds), inp=inp)
            report("denoise_streams_" + nm + "_per_stream_loop", ms_b, total, "blocks", bytes_a / F, flops,
                   "(b) one jdsp_denoise handle per stream, a loop of jdsp_denoise_process_dev from ctypes with precomputed "
                   "arguments: measured over %d streams and scaled by %d; %.1f x the streams entry"
                   % (n_loop, S // n_loop, ms_b / ms_a), inp=inp)
            report("denoise_streams_" + nm + "_stateless_batch", ms_c, total, "blocks", bytes_c / F, flops,
                   "(c) the yardstick: jdsp_denoise_batch_dev over the same chunks as utterances, nothing carried", inp=inp)
            for h in singles:
                h.close()
            d_a.close()
            d_c.close()
            del args_a, args_b, args_c, singles
        del ins, o16
    if on("mfcc"):
        x = torch.from_numpy(pcm_of(rng, 512 * (B + 1))).cuda()
        xr = rot(x)
        m = eng.mfcc()
        ms = timed(lambda: m.frames(xr(), B), a.iters)
        xs = x[:512 * 257].cpu().numpy()
        report("mfcc_native_1024_512_38ch", ms, B, "frames", 1024 + 96, 5 * 512 * 9 + 512 * 14 + 2 * 1024 + 2 * 38 * 12,
               "pre-emphasis/Hamming/FFT/mel/ln/DCT/lifter, 65,536 frames, 12 doubles out",
               cpu=cpu_rate(lambda: orc.mfcc_frames(orc.mfcc_native_cfg(), xs, 256), 256))
        m.close()
        x16 = torch.from_numpy(pcm_of(rng, 160 * (B - 1) + 400)).cuda()
        x16r = rot(x16)
        m = eng.mfcc(win_len=400, hop=160, n_fft=512, n_chan=40, n_cep=13, half_rate=8000.0)
        ms = timed(lambda: m.frames(x16r(), B), a.iters)
        report("mfcc_400_160_512fft_40mel", ms, B, "frames", 320 + 104, 5 * 512 * 9 + 512 * 14, "BASELINE config 4 framing")
        m.close()
    if on("mfcc10k"):
        # BASELINE config 4: a 10,000-utterance batch (ragged, 1-6 s at 16 kHz), every utterance framed
        # on its own; on N GPUs jeicyboodsp_amd.sharding.utterance_shard hands out whole utterances
        from jeicyboodsp_amd import sharding
        lens = rng.integers(16000, 96000, 10000)
        m = eng.mfcc(win_len=400, hop=160, n_fft=512, n_chan=40, n_cep=13, half_rate=8000.0)
        fpu = [(int(n) - 400) // 160 + 1 for n in lens]
        offs = np.concatenate([[0], np.cumsum(lens)])
        starts = np.concatenate([offs[u] + 160 * np.arange(fpu[u], dtype=np.int64) for u in range(len(lens))])
        x = torch.from_numpy(pcm_of(rng, int(offs[-1]))).cuda()
        st = torch.from_numpy(starts).cuda()
        ms = timed(lambda: m.frames(x, len(starts), frame_start=st), max(a.iters // 4, 3))
        loads = [sum(fpu[f:f + n]) for f, n in (sharding.utterance_shard(fpu, r, 8) for r in range(8))]
        report("mfcc_10k_utterances_400_160_512fft_40mel", ms, len(starts), "frames", 320 + 104, 5 * 512 * 9 + 512 * 14,
               "10,000 ragged utterances, %d frames; an 8-way utterance split is balanced to %.2f%%"
               % (len(starts), 100.0 * (max(loads) - min(loads)) / max(loads)))
        m.close()
    if on("gmm"):
        # the 10,000-utterance batch's MFCC vectors (12 cepstra, native MFCC configuration
        # framing is irrelevant here) scored where they lie: 25 classes (GMMTest:26) / one 6-state model (Viterbi:26-28)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import gmm_cases as gc
        fpu = rng.integers(98, 598, 10000)
        first = np.concatenate([[0], np.cumsum(fpu)]).astype(np.int64)
        nvec = int(first[-1])
        feats_h = rng.normal(0.0, 3.0, (nvec, 12))
        feats, first_d = torch.from_numpy(feats_h).cuda(), torch.from_numpy(first).cuda()
        classes = gc.gmm_records(1, 25)
        g = eng.gmm(classes)
        ms = timed(lambda: g.score(feats, first_d), max(a.iters // 8, 3))
        # per vector and class: 4 mixtures x (48 MAC + 4 x ~8 flops + 4 exp) + 1 log ~ 550 FP64 flops
        report("gmm_score_25_classes_10k_utterances", ms, nvec, "vectors", 96, 25 * 550,
               "FP64; %d vectors in 10,000 utterances against 25 four-mixture GMMs; flops are FP64" % nvec,
               cpu=cpu_rate(lambda: orc.gmm_classify(feats_h[:2000], classes), 2000))
        g.set_option("evaluation", 1)
        ms = timed(lambda: g.score(feats, first_d), max(a.iters // 8, 3))
        report("gmm_score_25_classes_10k_utterances_fused_evaluation", ms, nvec, "vectors", 96, 25 * 250,
               "opt-in: FMA projections, -0.5/var precomputed, one exp per mixture (jdsp_gmm_set_option evaluation=1)")
        g.close()
        models = gc.hmm_records(2, 1)
        h = eng.hmm(models)
        ms = timed(lambda: h.viterbi(feats, first_d, want_path=True), max(a.iters // 8, 3))
        report("hmm_recursion_6_states_10k_utterances", ms, nvec, "vectors", 96 + 4, 6 * 550,
               "FP64; emission kernel (vector-parallel) + one thread per utterance for the recursion",
               cpu=cpu_rate(lambda: orc.hmm_viterbi(feats_h[:20000], models[0]), 20000))
        h.close()
    if on("gmmtrain"):
        # GMM training (jdsp_gmm_trainer, GMMAlgorithm_Train_Auto_ver2.cpp): the gmm leg's ragged utterance lengths
        # (98..598 vectors, 10,000 files) as 25 classes x 400 files, trained in one call; vectors from 4 anisotropic
        # clusters per class (tests/gmm_train_cases.py) so that the kept eigen-subspaces are decided by the data
        import gmm_train_cases as gtc
        import gmm_train_ref as gtr
        feats_h, ff_h, fc_h = gtc.bench_files()
        nvec = int(ff_h[-1])
        feats = torch.from_numpy(feats_h).cuda()
        ff, fc = torch.from_numpy(ff_h).cuda(), torch.from_numpy(fc_h).cuda()
        tr = eng.gmm_trainer(25)
        tr.reserve(nvec, len(fc_h))

        def train_all():
            tr.reset()
            tr.train(feats, ff, fc)
        ms = timed(train_all, 1, rounds=3, spin_ms=0.0)
        # per vector: 3 EM iterations x (4 mixtures x (96 MAC + 8 exp + 8 x 4 flops) E-step + 52 MAC + 312 x 3 flops)
        n_cpu = int(ff_h[50])
        report("gmm_train_25_classes_400_files", ms, nvec, "vectors", 96 + 32, 3 * (4 * 300 + 104 + 936),
               "FP64; one workgroup per class over its 400 files (k-means, then 3 x (Jacobi -> E -> M) per file): "
               "%d vectors; ms is one full training from reset; bounded by the serial chain of 1,200 EM iterations "
               "per class, not by HBM; cpu_baseline: the numpy restatement (tests/gmm_train_ref.py) on the first "
               "50 files" % nvec,
               cpu=cpu_rate(lambda: gtr.train(feats_h[:n_cpu], ff_h[:51], fc_h[:50], 25), n_cpu))
        tr.close()
    if on("fastconv"):
        nb = 4096
        taps = rng.normal(size=7169) * 0.01
        x = torch.from_numpy(pcm_of(rng, nb * 1024, 2000.0)).cuda()
        fc = eng.fastconv(taps, 8192)

        fc.process(x)                                            # steady state: a stream fed 4,096 blocks per call
        ms = timed(lambda: fc.process(x), max(a.iters // 4, 3))
        xs = x[:71 * 1024].cpu().numpy()
        report("fastconv_8192_native", ms, nb, "blocks", 4096, 2 * 5 * 4096 * 12 + 2 * 4096 * 14 + 8192 * 6,
               "reference-native: 7169 taps, 1024-sample blocks, steady-state calls of 4,096 blocks; partitioned "
               "(15 x 512 taps) unless JDSP_FASTCONV_PARTITIONED=0; flops counted for the 8192-point formulation",
               cpu=cpu_rate(lambda: orc.fastconv_stream(xs, taps, 8192), 64))
        fc.close()
        nb = 65536
        h2 = rng.normal(size=(2, 256)) * 0.1
        x = torch.from_numpy(pcm_of(rng, nb * 769, 2000.0)).cuda()
        fc = eng.fastconv(h2, 1024)

        fc.process(x)
        xr = rot(x)
        ms = timed(lambda: fc.process(xr()), a.iters)
        xs = x[:513 * 769].cpu().numpy()
        report("fastconv_1024_hrir_pair", ms, nb, "blocks", 4614, 3 * 5 * 512 * 9 + 3 * 512 * 14 + 2 * 1024 * 6,
               "BASELINE config 2: 256-tap pair, 769-sample blocks, mono in -> 2 ears out",
               cpu=cpu_rate(lambda: [orc.fastconv_stream(xs, h2[0], 1024), orc.fastconv_stream(xs, h2[1], 1024)], 512))
        fc.close()
    if on("binaural"):
        # Live binaural rendering (jdsp_binaural_render_dev): 2,000 mixes x 8 sources x 2 blocks per delivery out of a
        # bank of 256 directions x 256 taps, 16,000 live streams.  Timed in this process, in alternated rounds, every C
        # entry called through ctypes with its arguments computed beforehand: (a) no stream fades; (a') every stream
        # moves in every delivery (the worst case: block 0 of every mix takes four inverse transforms); (b) today's
        # route -- one jdsp_fastconv handle per source (n_fft 1024, the direction's two filters zero-padded to 513 taps
        # so that its blocks are the same 512 samples) in a loop of _process_dev plus a torch sum per mix --, over the
        # first 25 mixes and scaled by 80; (c) the yardstick: BASELINE config 2's convolver leg as time per transform
        # (3 per block; (a) does S + 2 per block, (a') S + 4 for block 0 of a mix).  The inputs rotate over 9 copies of
        # 32.8 MB (295 MB, past the 256 MiB Infinity Cache).
        import ctypes as C
        from jeicyboodsp_amd import sharding
        from jeicyboodsp_amd._lib import lib as L
        M, S, NB, n_dirs, n_taps, n_loop_mixes = 2000, 8, 2, 256, 256, 25
        brng = np.random.default_rng(20)
        bank = brng.normal(size=(n_dirs, 2, n_taps)) * np.exp(-np.arange(n_taps) / 48.0) * 0.05
        hb = eng.binaural(bank)
        n_chunks, total = M * S, M * NB
        hb.open_streams(n_chunks)
        sf, cf, bf, _, n_samples = sharding.binaural_layout([NB] * M, [S] * M)
        vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
        d_ids = dev(brng.permutation(n_chunks).astype(np.int64))
        d_sf, d_cf, d_bf = dev(sf), dev(cf), dev(bf)
        dirs0 = brng.integers(0, n_dirs, n_chunks).astype(np.int32)
        d_dir = [dev(dirs0), dev((dirs0 + 1 + brng.integers(0, n_dirs - 1, n_chunks).astype(np.int32)) % n_dirs)]
        d_gain = dev(brng.uniform(0.1, 2.0, n_chunks).astype(np.float32))
        gen = torch.Generator(device="cuda").manual_seed(20)
        ins = [(torch.randn(n_samples, device="cuda", generator=gen) * 1500.0).round_().clamp_(-32768, 32767).to(torch.int16)
               for _ in range(1 if a.warm else 9)]
        plane = 512 * total
        o16 = torch.empty(2 * plane, dtype=torch.int16, device="cuda")
        args = [[(hb._h, vp(x), vp(d_ids), vp(d_sf), vp(d), vp(d_gain), vp(d_cf), vp(d_bf), M, n_chunks, total, vp(o16),
                  None, plane) for x in ins] for d in d_dir]
        # (b): the first n_loop_mixes mixes' sources, one handle each
        n_loop = n_loop_mixes * S
        padded = np.zeros((n_dirs, 2, 513))
        padded[:, :, :n_taps] = bank
        singles = [eng.fastconv(padded[dirs0[c]], 1024) for c in range(n_loop)]
        assert singles[0].block == 512
        b16 = torch.empty((n_loop, 2, NB * 512), dtype=torch.int16, device="cuda")
        args_b = [(h._h, vp(ins[0], 2 * int(sf[c])), NB, vp(b16[c]), None, None) for c, h in enumerate(singles)]
        # (c): config 2's convolver leg
        nb_c = 65536
        xc = torch.from_numpy(pcm_of(rng, nb_c * 769, 2000.0)).cuda()
        fcc = eng.fastconv(rng.normal(size=(2, 256)) * 0.1, 1024)
        xcr = rot(xc)
        eng._use_torch_stream()
        turn = [0, 0]

        def call_a():
            turn[0] += 1
            L.jdsp_binaural_render_dev(*args[0][turn[0] % len(ins)])

        def call_fade():
            turn[1] += 1
            L.jdsp_binaural_render_dev(*args[turn[1] & 1][turn[1] % len(ins)])

        def loop():
            for p in args_b:
                L.jdsp_fastconv_process_dev(*p)
            b16.view(n_loop_mixes, S, 2, NB * 512).sum(dim=1, dtype=torch.int32)

        def call_c():
            fcc.process(xcr())

        assert L.jdsp_binaural_render_dev(*args[0][0]) == 0 and L.jdsp_fastconv_process_dev(*args_b[0]) == 0
        for h in singles:                                        # past every handle's first block, which it drops
            L.jdsp_fastconv_process_dev(h._h, vp(ins[0]), 1, vp(b16), None, None)
        it = max(5 * a.iters, 20)
        ms_a, ms_f, ms_b, ms_c = timed_alternated([call_a, call_fade, loop, call_c], [it, it, 1, a.iters], rounds=5)
        ms_b *= M / n_loop_mixes
        tr_a, tr_f, tr_c = ms_a / (M * NB * (S + 2)), ms_f / (M * (NB * (S + 2) + 2)), ms_c / (nb_c * 3)
        inp = "rotated over %d copies of %.1f MB (from HBM)" % (len(ins), 2e-6 * n_samples)
        shape = "%d mixes x %d sources x %d blocks, bank %d directions x %d taps" % (M, S, NB, n_dirs, n_taps)
        tflops = lambda n_tr: n_tr * (5 * 512 * 9 + 512 * 14) + S * 2 * 640 * 8   # noqa: E731
        report("binaural_render", ms_a, total, "blocks", S * 1024 + 2 * 1024, tflops(S + 2),
               "(a) jdsp_binaural_render_dev, no stream fading: %s; %.2f ns per transform = %.3f x the config-2 convolver's "
               "%.2f ns (c); %.4f of the per-source loop (b); %d calls per round, 5 rounds"
               % (shape, 1e6 * tr_a, tr_a / tr_c, 1e6 * tr_c, ms_a / ms_b, it), inp=inp)
        report("binaural_render_all_fading", ms_f, total, "blocks", S * 1024 + 2 * 1024, tflops(S + 3),
               "(a') the same with every stream moving in every delivery: block 0 of every mix takes S + 4 transforms; "
               "%.2f ns per transform = %.3f x (c); %.3f x (a)" % (1e6 * tr_f, tr_f / tr_c, ms_f / ms_a), inp=inp)
        report("binaural_per_source_loop", ms_b, total, "blocks", S * 1024 + S * 2 * 1024, tflops(3 * S),
               "(b) today's route: one jdsp_fastconv handle per source (n_fft 1024, two filters, taps zero-padded to 513: blocks "
               "of 512) in a loop of jdsp_fastconv_process_dev from ctypes with precomputed arguments, and one torch sum "
               "per delivery over the sources of each mix: measured over %d mixes and scaled by %d; %.1f x (a)"
               % (n_loop_mixes, M // n_loop_mixes, ms_b / ms_a), inp=inp)
        report("binaural_yardstick_fastconv_1024_hrir_pair", ms_c, nb_c, "blocks", 4614, 3 * 5 * 512 * 9 + 3 * 512 * 14 + 2 * 1024 * 6,
               "(c) BASELINE config 2 in the same alternated rounds: %.2f ns per transform (3 per block)" % (1e6 * tr_c))
        for h in singles:
            h.close()
        fcc.close()
        hb.close()
        del ins, o16, b16, xc, xcr, args, args_b
    if on("fft"):
        n = 65536
        z = torch.from_numpy(rng.normal(size=(n, 512)) + 1j * rng.normal(size=(n, 512))).cuda()
        ms = timed(lambda: eng.fft_process(z), max(a.iters // 4, 3))
        zs = z[:256].cpu().numpy()
        report("fftprocess_f64_512", ms, n, "transforms", 2 * 512 * 16, 5 * 512 * 9, "FFTAlgorithm_ver2 FFTProcess, FP64, batch 65,536",
               cpu=cpu_rate(lambda: orc.fft_process(zs), 256))
    if on("pitch"):
        x = pcm_of(rng, B * 512)
        t = torch.from_numpy(x).cuda()
        tr_ = rot(t)
        ms = timed(lambda: eng.pitch(tr_()), a.iters)
        report("pitch_autocorr", ms, B, "blocks", 1024 + 8, 2 * 5 * 512 * 9 + 2 * 512 * 14,
               "PitchEstimation_method1 CalcPitch: FFT -> |X|^2 -> IFFT -> arg max, 65,536 blocks",
               cpu=cpu_rate(lambda: orc.pitch_stream(x[:1024 * 512]), 1024))
    # time-domain analysis (PitchEstimation_method2 / _method3, LPCEstimation): issue-bound, 1 KiB in per block
    td = [n for n in ("pitch_amdf", "pitch_acf", "lpc") if on(n)]
    if td:
        import timedomain_ref
        x = pcm_of(rng, B * 512)
        tr_ = rot(torch.from_numpy(x).cuda())
        slots = eng.n_cu * 64 * TD_CLOCK_GHZ * 1e9                 # lane-instructions per second of the whole chip
        for name, method, per_instr, instr in (("pitch_amdf", 2, 2, "v_sad_u16, two terms each"),
                                               ("pitch_acf", 3, 1, "FP64 FMA, one term each")):
            if name not in td:
                continue
            ms = timed(lambda: eng.pitch_lag(tr_(), method), max(a.iters // 4, 3))
            bound_ms = B * TD_TERMS_SEARCH / per_instr / slots * 1e3
            report(name, ms, B, "blocks", 1024 + 12, 2 * TD_TERMS_SEARCH,
                   "PitchEstimation_method%d CalcPitch, bit-exact, lags 101..511 (%d terms per block), 65,536 blocks; "
                   "issue bound (%s, %d CUs x 64 lanes x %.1f GHz) %.1f us = %.3f of the time"
                   % (method, TD_TERMS_SEARCH, instr, eng.n_cu, TD_CLOCK_GHZ, bound_ms * 1e3, bound_ms / ms),
                   cpu=cpu_rate(lambda: timedomain_ref.pitch_stream(x[:64 * 512], method), 64))
            ms = timed(lambda: eng.pitch_lag(tr_(), method, want_curve=True), max(a.iters // 4, 3))
            bound_ms = B * TD_TERMS_ALL / per_instr / slots * 1e3
            report(name + "_curve", ms, B, "blocks", 1024 + 12 + 4096, 2 * TD_TERMS_ALL,
                   "the same with the 512-lag curve written (%d terms and 4 KiB out per block); issue bound %.1f us = "
                   "%.3f of the time" % (TD_TERMS_ALL, bound_ms * 1e3, bound_ms / ms))
        if "lpc" in td:
            ms = timed(lambda: eng.lpc(tr_(), 256, 12), max(a.iters // 4, 3))
            report("lpc", ms, 2 * B, "blocks", 512 + 96, 2 * 13 * 512 + 2 * 12 ** 3 // 3 * 2,
                   "LPCEstimation: FP64 Hamming, 13 autocorrelation lags, 12x12 partial-pivot solve; 131,072 blocks of 256 "
                   "(the 65,536 x 512 samples of the pitch legs)",
                   cpu=cpu_rate(lambda: timedomain_ref.lpc_stream(x[:256 * 256], 256, 12), 256))
    # the sample-serial filters (7Band_GEQ, NormalLMS), batched over streams: one dependent FP64 chain per stream
    sf = [n for n in ("geq", "nlms") if on(n)]
    if sf:
        import streamfilter_ref
    if "geq" in sf:
        x = pcm_of(rng, B * 512, 1500.0).reshape(B, 512)
        xr = rot(torch.from_numpy(x).cuda())
        g = eng.geq(B)
        o16 = torch.empty((B, 512), dtype=torch.int16, device="cuda")
        ms = timed(lambda: g.process(xr(), out=o16), max(a.iters // 4, 3))
        co = streamfilter_ref.geq_design()
        report("geq", ms, B, "blocks", 2048, 7 * 512 * 10,
               "ApplyIirGEQ: 7 biquads, every section cast to int16, bit-exact; 65,536 streams x one reference block of 512 "
               "(8 lanes per stream, 8 streams per wave, 518 pipeline steps per call); flops are FP64; a single long stream "
               "runs at the latency of the per-step chain whatever the width of the GPU; cpu_baseline: the Python "
               "restatement (tests/streamfilter_ref.py)",
               cpu=cpu_rate(lambda: streamfilter_ref.geq(x[0], co), 1))
        g.close()
    if "nlms" in sf:
        ns, nblk = 4096, 16
        pairs = [streamfilter_ref.echo_pair(500 + i, nblk * 1024) for i in range(8)]
        xi = np.stack([pairs[i % 8][0] for i in range(ns)])
        xf = np.stack([pairs[i % 8][1] for i in range(ns)])
        xir, xfr = rot(torch.from_numpy(xi).cuda()), rot(torch.from_numpy(xf).cuda())
        f = eng.nlms(ns)
        o2 = (torch.empty((ns, nblk * 1024), dtype=torch.int16, device="cuda"),
              torch.empty((ns, nblk * 1024), dtype=torch.int16, device="cuda"))
        ms = timed(lambda: f.process(xir(), xfr(), out=o2), 2, rounds=3, spin_ms=0.0)
        report("nlms", ms, ns * nblk, "blocks", 3 * 2048, 1024 * (2 * 256 + 4 * 256),
               "LMSFilter: 256 taps, one wave per stream, bit-exact in the documented summation order; 4,096 streams x 16 "
               "blocks of 1,024 (16,384 serial steps per stream and call); flops are FP64, a division counted as one; a "
               "single long stream runs at the latency of the per-step chain; cpu_baseline: the numpy restatement "
               "(tests/streamfilter_ref.py)",
               cpu=cpu_rate(lambda: streamfilter_ref.nlms(pairs[0][0][:1024], pairs[0][1][:1024]), 1))
        f.close()
    if on("mvdr"):
        l = pcm_of(rng, B * 512)
        r = pcm_of(rng, B * 512)
        l[:12 * 512] = pcm_of(rng, 12 * 512, 45.0)
        tl, tr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
        mv = eng.mvdr(0.0)
        mv.process(tl, tr)
        tlr, trr = rot(tl), rot(tr)
        ms = timed(lambda: mv.process(tlr(), trr()), a.iters)
        report("mvdr_2mic", ms, B, "blocks", 3072, 3 * 5 * 512 * 9 + 3 * 512 * 14 + 1024 * 40,
               "BeamForming_MVDR_ver1: VAD + correlation + per-bin weights + inverse, 65,536 stereo blocks",
               cpu=cpu_rate(lambda: orc.mvdr_stream(l[:512 * 512], r[:512 * 512]), 512))
        mv.close()
    if on("mvdr8"):
        nbm = 16384
        mics = np.stack([pcm_of(rng, nbm * 512) for _ in range(8)])
        mics[:, :40 * 512] = np.stack([pcm_of(rng, 40 * 512, 30.0) for _ in range(8)])
        tm = torch.from_numpy(mics).cuda()
        mv = eng.mvdr_multi(8, None, 1e-3)
        mv.process(tm)

        ms = timed(lambda: mv.process(tm), max(a.iters // 4, 3))
        small = mics[:, :64 * 512].copy()
        report("mvdr_8mic_per_bin_covariance", ms, nbm, "blocks", 8 * 1024 + 1024, 9 * 5 * 512 * 9 + 9 * 512 * 14 + 1024 * 8 * 8,
               "BASELINE config 5 (generalisation, no reference): 8 microphones, per-bin 8x8 covariance, 16,384 blocks, 39 estimation frames",
               cpu=cpu_rate(lambda: orc.mvdrn_stream(small, None, 1e-3), 64))
        mv.close()
        # BASELINE config 5 as worded: 512-point frames (blocks of 256): 32,768 blocks = the same 8.4 M samples per microphone
        nb5 = 32768
        mv = eng.mvdr_multi(8, None, 1e-3, n_fft=512)
        mv.process(tm)
        ms = timed(lambda: mv.process(tm), max(a.iters // 4, 3))
        small5 = mics[:, :128 * 256].copy()
        report("mvdr_8mic_per_bin_covariance_512pt", ms, nb5, "blocks", 8 * 512 + 512, 4.5 * 5 * 512 * 9 + 1024 * 8 * 8 / 2,
               "BASELINE config 5 as worded (generalisation, no reference): 8 microphones, 512-point frames, per-bin 8x8 "
               "covariance over 257 bins, 32,768 blocks of 256, two microphones per forward and two blocks per inverse transform",
               cpu=cpu_rate(lambda: orc.mvdrn_stream(small5, None, 1e-3, n_fft=512), 128))
        mv.close()
    eng.close()


if __name__ == "__main__":
    main()
