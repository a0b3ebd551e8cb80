#!/usr/bin/env python3
"""Bit comparison of builds of libjdsp.so on the overlap-add, denoise, n-microphone MVDR and reverberation chains (GPU
box only):
    python tools/ab_bits.py build/variants/parent.so jeicyboodsp_amd/libjdsp.so ...
Every library runs in a fresh child process (JDSP_LIB) over the same seeded inputs and prints one SHA-256 per case over
the raw bytes of every output: int16, the float32 before the cast, the flushed tail and the recompute count where the
entry has them.  The parent prints the table and exits non-zero when a digest differs from the first library's.
    python tools/ab_bits.py --time ROUNDS LIB LIB ...
times the denoiser on the periodic stream (the only chain whose FP64 recompute pass runs: no benchmark leg has it),
the libraries alternated as named, ROUNDS times: median microseconds of 20 calls after 5."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def digest(*arrays):
    import numpy as np
    import torch
    h = hashlib.sha256()
    for a in arrays:
        if isinstance(a, torch.Tensor):
            a = a.cpu().numpy()
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def cut_calls(F, R):
    cuts = [1, R - 1, 7]
    return [c for c in cuts + [F - sum(cuts)] if c >= 0]


def geometries(R):
    return sorted({0, max(R - 1, 1), 5})


def synthesis(eng):
    import numpy as np
    import torch
    F = 29
    for n, hop in ((1024, 1024), (1024, 512), (1024, 256), (512, 512), (512, 256), (512, 128)):
        for layout in ("full", "half"):
            R = n // hop
            rng = np.random.default_rng(n + hop + len(layout))
            pitch = n if layout == "full" else n // 2 + 1
            x = (rng.normal(size=(F, pitch)) + 1j * rng.normal(size=(F, pitch))) * 3000.0 * np.sqrt(n) / 2
            spec = torch.from_numpy(x.astype(np.complex64)).cuda()
            ist = eng.istft(n_fft=n, hop=hop, layout=layout, synthesis_window="hann",
                            analysis_window="hann" if R > 1 else "none")
            for fpw in geometries(R):
                ist.set_option("frames_per_wave", fpw)
                outs, j = [], 0
                for c in cut_calls(F, R):
                    o, f = ist.process(spec[j:j + c], want_f32=True)
                    outs += [o.clone(), f.clone()]
                    j += c
                outs += list(ist.flush(want_f32=True))
                yield "istft %d/%d %s fpw %d" % (n, hop, layout, fpw), digest(*outs)
            ist.close()


def mask_cfg(hop, kind, combo):
    """StftMask's arguments for a (analysis, synthesis, normalise) combination, as the masking tests open it"""
    ana, syn, norm = combo
    return dict(n_fft=1024, hop=hop, analysis_window=ana, synthesis_window=syn, normalise=norm, mask_kind=kind)


def mask_streams():
    """(name, case) per hop and mask kind: the white stream and a notched tone known to recompute frames"""
    import stftmask_fp32_ref as S
    for c in S.cases():
        if c["white"] or c["name"].startswith(("notch_on", "notch_off", "local")):
            yield c


def masking(eng):
    import numpy as np
    import torch
    import stftmask_fp32_ref as S
    seen = set()
    for c in mask_streams():
        tag = ("white" if c["white"] else "tone", c["hop"], c["kind"])
        if tag in seen or c["mask_pitch"] == 0:
            continue
        seen.add(tag)
        hop, F, R = c["hop"], min(29, c["F"]), S.N // c["hop"]
        pcm, mask = torch.from_numpy(np.array(c["pcm"])).cuda(), torch.from_numpy(np.array(c["mask"])).cuda()
        sm = eng.stft_mask(**mask_cfg(hop, c["kind"], c["combo"]))
        for fpw in geometries(R):
            sm.set_option("frames_per_wave", fpw)
            outs, j, n_redo = [], 0, []
            for k in cut_calls(F, R):
                o, f = sm.process(pcm[hop * j:], mask[j:j + k], k, want_f32=True)
                outs += [o.clone(), f.clone()]
                n_redo.append(sm.frames_recomputed())
                j += k
            outs += list(sm.flush(want_f32=True))
            yield "stftmask %s fpw %d (%d recomputed)" % (c["name"], fpw, sum(n_redo)), digest(*outs, np.array(n_redo))
        sm.close()
    # tones exist for some (hop, kind) only: say which
    yield "stftmask streams", hashlib.sha256(repr(sorted(seen)).encode()).hexdigest()


def batches(eng):
    import numpy as np
    import torch
    import stftmask_fp32_ref as S
    from jeicyboodsp_amd import sharding
    for hop in (1024, 512, 256):
        R = 1024 // hop
        for counts in ([1, 0, R - 1, R, 2, 0, 0, 9, 1, 1, 37], [0, 0, 5, 4]):
            counts = np.array(counts, np.int64)
            rng = np.random.default_rng(hop + counts.size)
            packed, frame_first = sharding.istft_batch_layout(counts, 1024, hop)
            n_total = int(frame_first[-1])
            pcm = torch.from_numpy(np.clip(np.rint(rng.normal(0, 3000.0, int(packed[-1]))), -32768, 32767).astype(np.int16)).cuda()
            assert np.array_equal(sharding.stftmask_batch_layout(packed, 1024, hop)[0], counts)
            what = "hop %d x %d utterances" % (hop, counts.size)
            for fpw in geometries(R):
                eng.set_option("stft.frames_per_wave", fpw)
                spec = eng.stft_half_batch(pcm, packed, hop=hop, pitch=520)
                yield "stft_half_batch %s fpw %d" % (what, fpw), digest(torch.view_as_real(spec)[:, :513])
            eng.set_option("stft.frames_per_wave", 0)
            ist = eng.istft(n_fft=1024, hop=hop, layout="half", synthesis_window="hann",
                            analysis_window="hann" if R > 1 else "none")
            for fpw in geometries(R):
                ist.set_option("frames_per_wave", fpw)
                yield "istft_batch %s fpw %d" % (what, fpw), digest(*ist.process_batch(spec, counts, packed, want_f32=True))
            ist.close()
            for kind in ("real", "complex"):
                mask = torch.from_numpy(S.mask_of(rng, kind, n_total)).cuda()
                sm = eng.stft_mask(**mask_cfg(hop, kind, S.stream_combo(hop)))
                for fpw in geometries(R):
                    sm.set_option("frames_per_wave", fpw)
                    outs = sm.process_batch(pcm, mask, packed, want_f32=True)
                    yield "stftmask_batch %s %s fpw %d" % (what, kind, fpw), digest(*outs, np.array(sm.frames_recomputed()))
                sm.close()


def stream_calls(R):
    """Three calls of (stream, frames) chunks over five live streams: ids in no order, a stream or two absent from every
    call, chunks of 0, 1, R - 1, R and R + 1 frames"""
    return [[(3, R + 1), (0, 1), (4, 0), (1, R)],
            [(2, R - 1), (0, R), (3, 1)],
            [(4, R + 1), (1, 1), (0, R - 1), (2, R), (3, 0)]]


def stream_offsets(counts, n, hop, with_pcm, gaps):
    """the chunks' sample offsets: back to back, or pushed apart by even gaps that grow from chunk to chunk"""
    import numpy as np
    from jeicyboodsp_amd import sharding
    packed = sharding.stream_chunks_layout(counts, n, hop, with_pcm)[0]
    return packed + 2 * np.cumsum(np.arange(1, len(counts) + 1)) if gaps else packed


def streams(eng):
    """process_streams on both handles: the calls of stream_calls at every geometry, the second call at explicit offsets
    with gaps, then flush_streams of all five; once per handle with a process_batch and one of the handle's own
    process calls between the stream calls"""
    import numpy as np
    import torch
    import stftmask_fp32_ref as S
    N_LIVE = 5

    def totals(R):
        return [sum(f for call in stream_calls(R) for s, f in call if s == k) for k in range(N_LIVE)]

    for n, layout in ((1024, "half"), (1024, "full"), (512, "full")):
        for R in (1, 2, 4):
            hop = n // R
            rng = np.random.default_rng(7000 + n + hop + len(layout))
            pitch = n if layout == "full" else n // 2 + 1
            rows = [(rng.normal(size=(t, pitch)) + 1j * rng.normal(size=(t, pitch))) * 3000.0 * np.sqrt(n) / 2 for t in totals(R)]
            rows = [r.astype(np.complex64) for r in rows]
            own = torch.from_numpy(rows[0]).cuda()
            ist = eng.istft(n_fft=n, hop=hop, layout=layout, synthesis_window="hann",
                            analysis_window="hann" if R > 1 else "none")
            ist.open_streams(N_LIVE)
            for fpw in geometries(R) + ["interleaved"]:
                ist.set_option("frames_per_wave", 0 if fpw == "interleaved" else fpw)
                done, outs = [0] * N_LIVE, []
                for k, call in enumerate(stream_calls(R)):
                    counts = np.array([f for _, f in call], np.int64)
                    spec = np.concatenate([rows[s][done[s]:done[s] + f] for s, f in call] + [rows[0][:1]])
                    for s, f in call:
                        done[s] += f
                    first = stream_offsets(counts, n, hop, False, k == 1) if k == 1 else None
                    outs += [x.clone() for x in ist.process_streams(torch.from_numpy(spec).cuda(), [s for s, _ in call],
                                                                    counts, first, want_f32=True)]
                    if fpw == "interleaved" and k == 0:
                        outs += [x.clone() for x in ist.process_batch(own, [own.shape[0]], want_f32=True)]
                    if fpw == "interleaved" and k == 1:
                        outs += [x.clone() for x in ist.process(own, want_f32=True)]
                outs += list(ist.flush_streams(np.arange(N_LIVE), want_f32=True))
                if fpw == "interleaved":
                    outs += list(ist.flush(want_f32=True))
                yield "istft_streams %d/%d %s fpw %s" % (n, hop, layout, fpw), digest(*outs)
            ist.close()
    n = 1024
    for hop in (1024, 512, 256):
        R = n // hop
        for kind in ("real", "complex"):
            rng = np.random.default_rng(7100 + hop + len(kind))
            tot = totals(R)
            pcm = [np.clip(np.rint(rng.normal(0, 3000.0, hop * (t - 1) + n)), -32768, 32767).astype(np.int16) for t in tot]
            mask = [S.mask_of(rng, kind, t) for t in tot]
            own_pcm, own_mask = torch.from_numpy(pcm[0]).cuda(), torch.from_numpy(mask[0]).cuda()
            own_offs = np.array([0, pcm[0].size], np.int64)
            sm = eng.stft_mask(**mask_cfg(hop, kind, S.stream_combo(hop)))
            sm.open_streams(N_LIVE)
            for fpw in geometries(R) + ["interleaved"]:
                sm.set_option("frames_per_wave", 0 if fpw == "interleaved" else fpw)
                done, outs, n_redo = [0] * N_LIVE, [], []
                for k, call in enumerate(stream_calls(R)):
                    counts = np.array([f for _, f in call], np.int64)
                    at = stream_offsets(counts, n, hop, True, k == 1)
                    first = at if k == 1 else None                 # None: the handle packs them itself
                    buf = np.full(int(at[-1]) + hop * max(int(counts[-1]) - 1, 0) + n, 32767, np.int16)
                    for (s, f), a in zip(call, at):
                        if f:
                            buf[int(a):int(a) + hop * (f - 1) + n] = pcm[s][hop * done[s]:hop * (done[s] + f - 1) + n]
                    m = np.concatenate([mask[s][done[s]:done[s] + f] for s, f in call] + [mask[0][:1]])
                    for s, f in call:
                        done[s] += f
                    outs += [x.clone() for x in sm.process_streams(torch.from_numpy(buf).cuda(), torch.from_numpy(m).cuda(),
                                                                   [s for s, _ in call], counts, first, want_f32=True)]
                    n_redo.append(sm.frames_recomputed())
                    if fpw == "interleaved" and k == 0:
                        outs += [x.clone() for x in sm.process_batch(own_pcm, own_mask, own_offs, want_f32=True)]
                        n_redo.append(sm.frames_recomputed())
                    if fpw == "interleaved" and k == 1:
                        outs += [x.clone() for x in sm.process(own_pcm, own_mask, want_f32=True)]
                        n_redo.append(sm.frames_recomputed())
                outs += list(sm.flush_streams(np.arange(N_LIVE), want_f32=True))
                if fpw == "interleaved":
                    outs += list(sm.flush(want_f32=True))
                yield "stftmask_streams hop %d %s fpw %s" % (hop, kind, fpw), digest(*outs, np.array(n_redo))
            sm.close()


def periodic(n_fft):
    import denoise_fp32_ref as R
    return next(c for c in R.cases() if c["periodic"] and c["n_fft"] == n_fft)


def denoise(eng):
    import numpy as np
    for n_fft in (1024, 512):
        c = periodic(n_fft)
        B, nb = c["block"], c["pcm"].size // c["block"]
        d = eng.denoiser(0, n_fft, B)
        outs, n_redo = [], []
        for a, b in ((0, nb // 2), (nb // 2, nb)):
            outs += list(d.process(c["pcm"][a * B:b * B], want_precast=True))
            n_redo.append(d.frames_recomputed())
        d.close()
        assert sum(n_redo) > 0
        yield "denoise %s in two calls (%d recomputed)" % (c["name"], sum(n_redo)), digest(*outs, np.array(n_redo))
    yield from denoise_batches(eng)
    yield from denoise_streams(eng)


BPW = (0, 1, 4)          # the denoiser's blocks_per_wave: one round of resident waves, a wave per block, four blocks


def speechlike_pcm():
    """130 blocks of voice and pauses: one of the white streams of the denoise tests"""
    import denoise_fp32_ref as R
    return R.white_pcm(next(w for w in R.WHITE_STREAMS if w[:3] == (512, 9, 130)))


def denoise_batches(eng):
    """process_batch in both modes: utterances cut from the periodic stream (frames go to the FP64 pass) and from a
    speech-like one (utterances of 0, 1, 2 and 3 blocks, one over the 64 blocks a wave ballots at a time)"""
    import numpy as np
    c, sp = periodic(1024), speechlike_pcm()
    nb = c["pcm"].size // 512
    cuts = 512 * np.cumsum([0, 70, 0, 1, 2, 3, 12])
    batches = ((c["name"], [c["pcm"][:k * 512] for k in (nb, nb - 7, nb // 2 + 3)]),
               ("speechlike", [sp[a:b] for a, b in zip(cuts[:-1], cuts[1:])]))
    for mode in (0, 1):
        for name, utts in batches:
            counts = [u.size // 512 for u in utts]
            d = eng.denoiser(mode, 1024, 512)
            for bpw in BPW:
                d.set_option("blocks_per_wave", bpw)
                outs = d.process_batch(np.concatenate(utts), counts, want_precast=True, want_flags=True, want_noise=True)
                n_redo = d.frames_recomputed()
                assert mode or name == "speechlike" or n_redo > 0
                yield ("denoise_batch mode %d %s x %d utterances bpw %d (%d recomputed)" % (mode, name, len(utts), bpw, n_redo),
                       digest(*outs, np.array(n_redo)))
            d.close()


def denoise_stream_calls():
    """(stream, blocks) chunks over five live streams: ids in no order, a stream or two absent from every call, chunks
    of 0, 1, 2, 3, 12 and 70 blocks (70: over the 64 blocks a wave ballots at a time); then stream 0 a block per call
    through its periodic stretch, where every frame is the first and the last of its chunk"""
    return [[(3, 2), (0, 12), (4, 0), (1, 1)],
            [(2, 70), (0, 3), (3, 1), (1, 2)],
            [(4, 12), (1, 70), (0, 1), (2, 0), (3, 3)],
            [(0, 2), (2, 12), (4, 3)]] + [[(0, 1)]] * 10


def denoise_streams(eng):
    """process_streams in both modes at every blocks_per_wave.  Streams 0..3 read the periodic stream, repeated, from
    the blocks 0, 5, 0 and 13 on; stream 4 the speech-like one.  Handed over: list entries of the live calls beyond
    those of process_batch over each stream's whole history, i.e. frames whose second block came with the next call."""
    import numpy as np
    N_LIVE, calls = 5, denoise_stream_calls()
    c = periodic(1024)
    tiled = np.tile(c["pcm"], 3)
    src = [tiled[512 * at:] for at in (0, 5, 0, 13)] + [speechlike_pcm()]
    total = [sum(n for call in calls for s, n in call if s == k) for k in range(N_LIVE)]
    assert all(3 <= t <= x.size // 512 for t, x in zip(total, src))
    for mode in (0, 1):
        d = eng.denoiser(mode, 1024, 512)
        d.process_batch(np.concatenate([x[:512 * t] for x, t in zip(src, total)]), total)
        n_batch = d.frames_recomputed()
        for bpw in BPW:
            d.set_option("blocks_per_wave", bpw)
            d.open_streams(N_LIVE, 160)                          # every stream fresh again
            done, outs, n_redo = [0] * N_LIVE, [], []
            for call in calls:
                pcm = np.concatenate([src[s][512 * done[s]:512 * (done[s] + n)] for s, n in call])
                for s, n in call:
                    done[s] += n
                outs += list(d.process_streams(pcm, [s for s, _ in call], [n for _, n in call], want_precast=True,
                                               want_flags=True))
                n_redo.append(d.frames_recomputed())
            outs += list(d.streams_state(np.arange(N_LIVE)))
            handed = sum(n_redo) - n_batch
            assert mode or (n_batch > 0 and handed > 0), (n_batch, n_redo)
            yield ("denoise_streams mode %d bpw %d (%d recomputed, %d handed over)" % (mode, bpw, sum(n_redo), handed),
                   digest(*outs, np.array(n_redo)))
        d.close()


def mvdrn(eng):
    """The n-microphone MVDR, stream and batch.  Stream: a 40-block scene in calls of 1 + 11 + 28 blocks of 512 samples
    (the carried block, the carried covariance and version 0 of a later call), at both loadings (0: a singular lead, NaN
    frames) and both frame lengths (the 512-point path shares the update kernel); a steering of fractional delays; and
    quiet runs of 129 and 300 estimation frames in one call (two and three events per chunk).  Batch: the
    oracle-per-utterance batch, quiet runs around the chunk length P between two ordinary utterances, the fractional
    steering, loading 0, and a batch with gaps on planes wider than their samples."""
    import numpy as np
    import torch
    import mvdrn_batch_cases as K
    from mvdrn_cases import steering_delays

    def stream(name, pcm, delays, loading, n_fft, cuts):
        h = eng.mvdr_multi(pcm.shape[0], delays, loading, n_fft)
        outs, at = [], 0
        for c in cuts:
            outs += list(h.process(pcm[:, K.B * at:K.B * (at + c)], want_precast=True))
            at += c
        h.close()
        return "mvdrn %s, %d mics, %d-point, loading %g, calls %s" % (name, pcm.shape[0], n_fft, loading, list(cuts)), digest(*outs)

    for n_fft, n_mics in ((1024, 2), (1024, 3), (1024, 8), (512, 3), (512, 8)):
        pcm, _, delays = K.array_scene(40 + n_mics, n_mics, 40)
        for loading in (K.LOADING, 0.0):
            yield stream("array_scene", pcm, delays, loading, n_fft, (1, 11, 28))
    pcm = K.array_scene(48, 8, 40)[0]
    yield stream("array_scene steering_frac", pcm, steering_delays("steering_frac", 8), K.LOADING, 1024, (1, 11, 28))
    for n_events in (129, 300):
        pcm = K.events_run(n_events, n_events)
        for n_fft in (1024, 512):
            yield stream("events_run %d" % n_events, pcm, K.delays_of(3), K.LOADING, n_fft, (pcm.shape[1] // K.B,))

    def batch(name, utts, delays, loading, gaps=None, wider=0):
        pcm, counts, first = K.pack(utts, gaps, pad=8 if wider else 0)
        planes = torch.zeros(pcm.shape[0], pcm.shape[1] + wider, dtype=torch.int16).cuda()
        planes[:, :pcm.shape[1]] = torch.from_numpy(pcm)
        h = eng.mvdr_multi(pcm.shape[0], delays, loading)
        outs = h.process_batch(planes[:, :pcm.shape[1]], counts, first, want_precast=True, want_flags=True)
        h.close()
        return "mvdrn_batch %s, %d mics x %d utterances, loading %g" % (name, pcm.shape[0], len(utts), loading), digest(*outs)

    for n_mics in (3, 8):
        yield batch("oracle_batch_utts", K.oracle_batch_utts(n_mics), K.delays_of(n_mics), K.LOADING)
    for n_events in (K.P - 1, K.P, K.P + 1, 2 * K.P + 1):
        utts = [K.utterance(1, 3, 12), K.events_run(n_events, n_events), K.utterance(2, 3, 12)]
        yield batch("events_run %d" % n_events, utts, K.delays_of(3), K.LOADING)
    utts = K.oracle_batch_utts(3)
    yield batch("steering_frac", utts, steering_delays("steering_frac", 3), K.LOADING)
    yield batch("oracle_batch_utts", utts, K.delays_of(3), 0.0)
    yield batch("gaps, chan_stride + 64", utts, K.delays_of(3), K.LOADING, gaps=2 * np.arange(len(utts)), wider=64)


def reverb(eng):
    """The reverberator, batch and live, on the device entries.  Batch: every bank of tests/reverb_cases.banks() over
    its batch (plan_of: utterances of 0, 1, 2, P - 1 .. P + 2, G - 1, G, G + 1 and 2 G + 1 blocks), spans apart by gaps_of.
    Streams: all streams of tests/reverb_streams_cases of the bank side by side, the constant ones under one cut pattern
    per case (the switched ones keep their own cuts), then the state of every stream."""
    import numpy as np
    import torch
    import reverb_cases as K
    import reverb_streams_cases as S
    for name, taps in K.banks().items():
        rv = eng.reverb(taps)
        plan = K.plan_of(rv.n_part, rv.n_irs)
        xs = [K.utterance(fam, nb, i) for i, (fam, nb, _, _) in enumerate(plan)]
        pcm, first, block_first = K.pack(xs, K.gaps_of(len(xs)), fill=32767)
        outs = rv.process_batch(torch.from_numpy(pcm).cuda(), first, block_first, [p[2] for p in plan], [p[3] for p in plan],
                                want_f32=True)
        yield "reverb_batch %s, P %d x %d utterances" % (name, rv.n_part, len(xs)), digest(*outs)
        strs = S.streams(name)
        rv.open_streams(len(strs), sum(s.x.size // S.B for s in strs))
        for pattern in S.PATTERNS:
            rv.reset_streams()
            outs = []
            for t, chunks in enumerate(S.deliveries(strs, rv.n_part, [pattern] * len(strs), len(pattern))):
                pcm, first, counts = S.pack_call(strs, chunks, K.gaps_of(len(chunks)), tail=2 * (t % 3))
                outs += [x.clone() for x in rv.process_streams(torch.from_numpy(pcm).cuda(), [c.stream for c in chunks], counts,
                                                               [c.ir for c in chunks], [c.gain for c in chunks], first,
                                                               want_f32=True)]
            outs += list(rv.streams_state(np.arange(len(strs))))
            yield "reverb_streams %s, P %d x %d streams, %s" % (name, rv.n_part, len(strs), pattern), digest(*outs)
        rv.close()


def child():
    import jeicyboodsp_amd
    eng = jeicyboodsp_amd.Engine(0)
    if sys.argv[2:3] == ["time"]:
        import statistics
        import time
        import numpy as np
        import torch
        c = periodic(1024)
        pcm = torch.from_numpy(np.array(c["pcm"])).cuda()
        d = eng.denoiser(0, 1024, 512)
        t = []
        for i in range(25):
            d.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.process(pcm)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e6)
        print("%s\t%.1f" % (c["name"], statistics.median(t[5:])))
        d.close()
    else:
        for chain in (synthesis, masking, batches, streams, denoise, mvdrn, reverb):
            for name, sha in chain(eng):
                print("%s\t%s" % (name, sha), flush=True)
    eng.close()


def run_child(lib, *args):
    env = dict(os.environ, JDSP_LIB=os.path.abspath(lib))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + list(args), env=env, check=True,
                         stdout=subprocess.PIPE, text=True, timeout=600).stdout
    return [line.split("\t") for line in out.splitlines() if "\t" in line]


def main():
    if sys.argv[1] == "--child":
        return child()
    if sys.argv[1] == "--time":
        for r in range(int(sys.argv[2])):
            for lib in sys.argv[3:]:
                for name, us in run_child(lib, "time"):
                    print("round %d  %-40s %-24s %9s us" % (r, lib, name, us), flush=True)
        return 0
    libs = sys.argv[1:]
    tables = [run_child(lib) for lib in libs]
    assert all(len(t) == len(tables[0]) for t in tables), [len(t) for t in tables]
    bad = 0
    for rows in zip(*tables):
        names, shas = {r[0] for r in rows}, [r[1] for r in rows]
        same = len(names) == 1 and len(set(shas)) == 1
        bad += not same
        print("%-64s %s  %s" % (rows[0][0], "  ".join(s[:16] for s in shas), "equal" if same else "DIFFER"))
    print("%d cases, %d libraries: %s" % (len(tables[0]), len(libs), "FAIL: %d differ" % bad if bad else "all equal"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
