"""Live multi-stream spectral subtraction / Wiener (jdsp_denoise_streams*, Denoiser.process_streams): chunks that
continue streams whose state is carried on the device.

The yardstick of every test is Denoiser.process_batch on a fresh handle with the stream's WHOLE history as one
utterance: the stream's emitted blocks, concatenated over its calls, equal the batch's output blocks 1 .. B - 2, its
flags the batch's flags, its estimate the batch's noise_last -- with np.array_equal, on the bits.  The deliveries go
through the device entry with sentinel-filled outputs, so what a call must not write is checked at every call."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_fp32_ref as R
from test_denoise_batch_gpu import SENT_F, SENT_I, loud, quiet, vp
from test_denoise_gpu import check_stream, speechlike

pytestmark = pytest.mark.gpu

B = 512
GAPS = (0, 2, 514)


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def lib():
    from jeicyboodsp_amd._lib import lib as L
    return L


_YARD = {}


def yardstick(eng, mode, pcm):
    """(emitted int16, emitted float32, flags, noise_last, frames recomputed) of pcm as ONE utterance of a fresh handle's
    process_batch, the output moved from time-aligned to stream order; computed once per (mode, samples), read-only"""
    key = (mode, pcm.tobytes())
    if key not in _YARD:
        nb = pcm.size // B
        d = eng.denoiser(mode)
        out, pre, flags, noise = d.process_batch(pcm, [nb], want_precast=True, want_flags=True, want_noise=True)
        n_redo = d.frames_recomputed()
        d.close()
        e = max(nb - 2, 0)
        res = (out[B:B + e * B].copy(), pre[B:B + e * B].copy(), flags.copy(), noise[0].copy(), n_redo)
        for a in res[:4]:
            a.setflags(write=False)
        _YARD[key] = res
    return _YARD[key]


def run_lengths(flags):
    """main()'s iNumOfIteration after every block (SS:98-109)"""
    r, out = 0, []
    for f in flags:
        r = 0 if f else r + 1
        out.append(r)
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


class Live:
    """A handle's live streams, fed through jdsp_denoise_streams_dev; keeps what every stream was given and gave."""

    def __init__(self, eng, mode, n_streams, max_blocks, bpw=0):
        self.eng, self.n_streams = eng, n_streams
        self.d = eng.denoiser(mode)
        if bpw:
            self.d.set_option("blocks_per_wave", bpw)
        self.d.open_streams(n_streams, max_blocks)
        self.fed = {s: [] for s in range(n_streams)}           # the blocks' samples
        self.got_i = {s: [] for s in range(n_streams)}
        self.got_f = {s: [] for s in range(n_streams)}
        self.flags = {s: [] for s in range(n_streams)}
        self.n_redo = 0

    def seen(self, s):
        return sum(x.size for x in self.fed[s]) // B

    def forget(self, ids):
        for s in ids:
            self.fed[s], self.got_i[s], self.got_f[s], self.flags[s] = [], [], [], []

    def deliver(self, chunks, gap=0, lead=0, out=True, pre=True, flags=True, emitted=True):
        """chunks: [(stream, int16 samples of whole blocks)] in the call's order.  Spans `gap` apart in a buffer of
        full-scale samples; outputs start as sentinels.  Checks n_emitted and everything no chunk may write."""
        import torch
        from jeicyboodsp_amd.sharding import denoise_stream_emitted
        L = lib()
        ids = np.array([s for s, _ in chunks], np.int64)
        counts = np.array([x.size // B for _, x in chunks], np.int64)
        starts, pos = [], lead
        for _, x in chunks:
            starts.append(pos)
            pos += x.size + gap
        n_samples, n_total = max(pos, 1), int(counts.sum())
        pcm = np.full(n_samples, 32767, np.int16)
        for st, (_, x) in zip(starts, chunks):
            pcm[st:st + x.size] = x
        block_first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
        full = lambda n, v, dt: torch.full((max(n, 1),), v, dtype=dt, device="cuda")     # noqa: E731
        d_pcm, d_id, d_s, d_b = t(pcm), t(ids), t(np.array(starts, np.int64)), t(block_first)
        d_o = full(n_samples, int(SENT_I), torch.int16) if out else None
        d_p = full(n_samples, float(SENT_F), torch.float32) if pre else None
        d_f = full(n_total, 77, torch.uint8) if flags else None
        d_e = full(len(chunks), -5, torch.int64) if emitted else None
        self.eng._use_torch_stream()
        rc = L.jdsp_denoise_streams_dev(self.d._h, vp(d_pcm), vp(d_id), vp(d_s), vp(d_b), len(chunks), n_total, vp(d_o),
                                        vp(d_p), vp(d_f), vp(d_e))
        assert rc == 0, L.jdsp_last_error(self.eng._h)
        torch.cuda.synchronize()
        self.n_redo += self.d.frames_recomputed()
        want_e = denoise_stream_emitted([self.seen(s) for s in ids], counts)
        if emitted and n_total and len(chunks):
            assert np.array_equal(d_e.cpu().numpy(), want_e), "n_emitted"
        o = d_o.cpu().numpy() if out else None
        p = d_p.cpu().numpy() if pre else None
        f = d_f.cpu().numpy() if flags else None
        covered = np.zeros(n_samples, bool)
        for c, (s, x) in enumerate(chunks):
            a, n = starts[c], int(want_e[c]) * B
            covered[a:a + n] = True
            if out:
                self.got_i[s].append(o[a:a + n].copy())
            if pre:
                self.got_f[s].append(p[a:a + n].copy())
            if flags:
                self.flags[s].append(f[block_first[c]:block_first[c + 1]].copy())
            if x.size:
                self.fed[s].append(x)
        if out:
            assert np.all(o[~covered] == SENT_I), "int16 written outside what the chunks emit"
        if pre:
            assert np.all(p[~covered] == SENT_F), "float32 written outside what the chunks emit"

    def check(self, mode, streams=None, what=""):
        """every stream against the batch yardstick on everything it was fed"""
        streams = list(range(self.n_streams)) if streams is None else list(streams)
        noise, seen = self.d.streams_state(streams)
        for k, s in enumerate(streams):
            nb = self.seen(s)
            assert seen[k] == nb, (what, s, "blocks seen")
            if nb == 0:
                assert not noise[k].any(), (what, s)
                continue
            y_i, y_f, y_flags, y_noise, _ = yardstick(self.eng, mode, np.concatenate(self.fed[s]))
            assert np.array_equal(np.concatenate(self.got_i[s]), y_i), (what, s, "int16")
            assert same_bits(np.concatenate(self.got_f[s]), y_f), (what, s, "float32")
            assert np.array_equal(np.concatenate(self.flags[s]), y_flags), (what, s, "flags")
            assert same_bits(noise[k], y_noise), (what, s, "estimate")

    def close(self):
        self.d.close()


def blocks_of(pcm, a, b):
    return pcm[a * B:b * B]


# ---- 1. cuts -----------------------------------------------------------------------------------------------------------
N_STREAMS = 9            # seven are fed; the ids include n_streams - 1


@functools.lru_cache(maxsize=None)
def cut_streams():
    """id -> (samples, chunk sizes).  Quiet leads put the run lengths where the cuts are, by construction; the test
    asserts them from the batch's flags."""
    rng = np.random.default_rng(190)
    cuts = np.random.default_rng(191)

    def random_cuts(n, hi):
        out = []
        while sum(out) < n:
            out.append(min(int(cuts.integers(0, hi + 1)), n - sum(out)))
        return out

    st = {}
    # 0: one block per call throughout; two latches
    x = np.concatenate([quiet(rng, 12), loud(rng, 5), quiet(rng, 14), loud(rng, 4), speechlike(21, 10)])
    st[0] = (x, [1] * (x.size // B))
    # 8 (= n_streams - 1): a first chunk of 1 block (stash only) cuts between run length 1 and 2; the next cut lies
    # between run length 9 and 10: the latch falls on a chunk's first block
    x = np.concatenate([quiet(rng, 13), loud(rng, 6), speechlike(22, 21)])
    st[8] = (x, [1, 8, 4, 0, 3] + random_cuts(x.size // B - 16, 5))
    # 2: a first chunk of 2 blocks (computed but discarded); then a latch in the middle of a chunk, twice: from no
    # estimate to the first and from the first to the second
    x = np.concatenate([quiet(rng, 12), loud(rng, 3), quiet(rng, 13), loud(rng, 5), speechlike(23, 12)])
    st[2] = (x, [2, 12, 6, 11] + random_cuts(x.size // B - 31, 4))
    # 3: a first chunk of 3 blocks (the first emission)
    x = speechlike(24, 41)
    st[3] = (x, [3] + random_cuts(41 - 3, 6))
    # 4: more than 64 blocks, most of them in ONE chunk: the noise pass walks the flags 64 at a time
    x = speechlike(25, 75, pattern=[11, 4, 13, 3, 2, 5, 12, 6])
    st[4] = (x, [1, 70, 0, 4])
    # 5, 6: speechlike, seeded random cuts with empty chunks
    st[5] = (speechlike(26, 52), random_cuts(52, 7))
    st[6] = (speechlike(27, 40, pattern=[3, 2, 14, 1, 10, 6]), random_cuts(40, 3))
    for x, c in st.values():
        assert sum(c) == x.size // B and 40 <= x.size // B <= 75
    return st


def test_the_cuts_reach_every_run_length_situation(eng):
    """from the batch's own flags: the situations test_cuts is meant to contain are in it"""
    st = cut_streams()
    for mode in (0, 1):
        r = {s: run_lengths(yardstick(eng, mode, x)[2]) for s, (x, _) in st.items()}
        starts = {s: np.concatenate([[0], np.cumsum(c)]) for s, (_, c) in st.items()}
        assert set(st[0][1]) == {1}                                          # one block per call throughout
        assert [st[8][1][0], st[2][1][0], st[3][1][0]] == [1, 2, 3]          # first chunks of 1, 2 and 3 blocks
        assert r[8][0] == 1 and r[8][1] == 2 and starts[8][1] == 1           # a cut between run length 1 and 2
        assert r[8][8] == 9 and r[8][9] == 10 and 9 in starts[8]             # ... and between 9 and 10
        inside = [(a, b, i) for a, b in zip(starts[2][:-1], starts[2][1:]) for i in range(a + 1, b) if r[2][i] == 10]
        assert len(inside) >= 2, inside                                      # a latch in the middle of a chunk
        assert max(st[4][1]) > 64 and st[4][0].size // B > 64
        assert any(c >= 3 for _, cs in st.values() for c in cs)              # several waves share a chunk at 1 block per wave
        assert any(c == 0 for _, cs in st.values() for c in cs)


@pytest.mark.parametrize("bpw", [0, 1, 2, 4, 8])
@pytest.mark.parametrize("mode", [0, 1])
def test_cuts(eng, mode, bpw):
    """Seven streams cut into chunks of 0, 1, 2, 3, ... blocks, dealt over calls with a random subset of the streams
    and a random chunk order per call; the gaps between the spans (0, 2, 514 samples, by turns) are full scale."""
    st = cut_streams()
    deal = np.random.default_rng(192 + bpw)
    lv = Live(eng, mode, N_STREAMS, 160, bpw)
    todo = {s: list(c) for s, (_, c) in st.items()}
    at = {s: 0 for s in st}
    call = 0
    while any(todo.values()):
        ids = [s for s in st if todo[s] and (s == 0 or deal.random() < 0.6)]
        deal.shuffle(ids)
        chunks = []
        for s in ids:
            n = todo[s].pop(0)
            chunks.append((s, blocks_of(st[s][0], at[s], at[s] + n)))
            at[s] += n
        lv.deliver(chunks, gap=GAPS[call % 3], lead=(call % 2) * 4)
        call += 1
    assert call >= 40
    lv.check(mode, what=(mode, bpw))
    untouched, seen = lv.d.streams_state([1, 7])
    assert not untouched.any() and not seen.any()
    lv.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_one_live_stream(eng, mode):
    """n_streams = 1"""
    x = speechlike(31, 33)
    lv = Live(eng, mode, 1, 16)
    a = 0
    for n in (1, 0, 2, 7, 1, 16, 3, 3):
        lv.deliver([(0, blocks_of(x, a, a + n))], gap=2)
        a += n
    assert a == 33
    lv.check(mode)
    lv.close()


# ---- 2. the FP64 hand-over ---------------------------------------------------------------------------------------------
def periodic_cases(eng):
    """the periodic 1024-point streams whose batch sends frames to the FP64 pass"""
    return [c for c in R.cases() if c["n_fft"] == 1024 and c["periodic"] and yardstick(eng, 0, c["pcm"])[4] > 0]


def test_fp64_hand_over(eng):
    """Spectral subtraction on periodic input, one stream per way of cutting: one block per call (every frame is first
    and last of its chunk), twos at both phases, threes at every phase."""
    cases = periodic_cases(eng)
    assert len(cases) >= 1
    for c in cases:
        x, nb = c["pcm"], c["pcm"].size // B
        assert yardstick(eng, 0, x)[4] > 0
        plans = [[1] * nb]
        for size in (2, 3):
            for phase in range(size):
                p = ([phase] if phase else []) + [size] * ((nb - phase) // size)
                plans.append(p + ([nb - sum(p)] if nb > sum(p) else []))
        assert all(sum(p) == nb for p in plans)
        lv = Live(eng, 0, len(plans), 3 * len(plans))
        at = [0] * len(plans)
        while any(plans):
            chunks = []
            for s, p in enumerate(plans):
                if p:
                    n = p.pop(0)
                    chunks.append((s, blocks_of(x, at[s], at[s] + n)))
                    at[s] += n
            lv.deliver(chunks)
        assert lv.n_redo > 0, c["name"]
        lv.check(0, what=c["name"])
        lv.close()


# ---- 3. one stream against the oracle directly ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_against_the_oracle(eng, oracle, mode):
    x = speechlike(140, 40)
    o_out, o_pre, o_flags, noises, ver = oracle.denoise_trace(mode, x)
    lv = Live(eng, mode, 3, 12)
    a = 0
    for n in (1, 1, 1, 5, 2, 12, 0, 7, 3, 8):
        lv.deliver([(1, blocks_of(x, a, a + n))])
        a += n
    assert a == 40
    check_stream(np.concatenate(lv.got_i[1]), np.concatenate(lv.got_f[1]), o_out, o_pre)
    assert np.array_equal(np.concatenate(lv.flags[1]).astype(np.int32), o_flags)
    noise, seen = lv.d.streams_state([1])
    assert seen[0] == 40
    assert np.abs(noise[0] - noises[-1]).max() <= 1e-5 * max(noises[-1].max(), 1.0)
    lv.close()


# ---- 4. what is not written ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_absent_streams_and_empty_chunks_change_nothing(eng, mode):
    """(the sentinels outside the emitted blocks and n_emitted are checked by every delivery of this file)"""
    x, y = speechlike(41, 30), speechlike(42, 30)
    lv = Live(eng, mode, 4, 40)
    lv.deliver([(0, blocks_of(x, 0, 14)), (2, blocks_of(y, 0, 13))])
    before = lv.d.streams_state([0, 1, 2, 3])
    lv.deliver([(2, blocks_of(y, 13, 13)), (0, blocks_of(x, 14, 14))])       # chunks of no blocks
    lv.deliver([(3, blocks_of(x, 0, 0))])
    after = lv.d.streams_state([0, 1, 2, 3])
    assert same_bits(before[0], after[0]) and np.array_equal(before[1], after[1])
    lv.deliver([(0, blocks_of(x, 14, 20))])                                  # stream 2 is absent
    mid = lv.d.streams_state([2])
    assert same_bits(mid[0], before[0][2:3]) and mid[1][0] == 13
    lv.deliver([(2, blocks_of(y, 13, 30)), (0, blocks_of(x, 20, 30))])
    lv.check(mode)
    # n_chunks == 0 and n_blocks_total == 0 launch nothing
    L = lib()
    assert L.jdsp_denoise_streams_dev(lv.d._h, None, None, None, None, 0, 0, None, None, None, None) == 0
    lv.check(mode)
    lv.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_null_outputs_advance_the_state(eng, mode):
    """with out and precast NULL the state advances exactly as with them"""
    x, y = R.cases()[1]["pcm"] if mode == 0 else speechlike(43, 35), speechlike(44, 35)
    nb = min(x.size, y.size) // B
    cuts = [3, 1, 9, 2, 4, 1, 6, nb - 26]
    full, part = Live(eng, mode, 2, 24), Live(eng, mode, 2, 24)
    a = 0
    for k, n in enumerate(cuts):
        chunks = [(1, blocks_of(x, a, a + n)), (0, blocks_of(y, a, a + n))]
        full.deliver(chunks)
        blind = k in (1, 2, 5)
        part.deliver(chunks, out=not blind, pre=not blind, flags=not blind)
        a += n
        sf, sp = full.d.streams_state([0, 1]), part.d.streams_state([0, 1])
        assert same_bits(sf[0], sp[0]) and np.array_equal(sf[1], sp[1]), k
        if not blind:
            for s in (0, 1):
                assert np.array_equal(full.got_i[s][k], part.got_i[s][-1]), (k, s)
                assert same_bits(full.got_f[s][k], part.got_f[s][-1]), (k, s)
    full.check(mode)
    full.close()
    part.close()


# ---- 5. reset --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_reset_and_the_other_entries_of_the_handle(eng, mode):
    xs = [speechlike(50 + s, 36) for s in range(4)]
    own_pcm = speechlike(60, 24)
    ref = eng.denoiser(mode)
    want_own = [ref.process(own_pcm[:9 * B], want_precast=True), ref.process(own_pcm[9 * B:], want_precast=True)]
    want_batch = ref.process_batch(xs[0], [20, 16], want_precast=True, want_flags=True, want_noise=True)
    ref.close()
    lv = Live(eng, mode, 4, 64)
    lv.deliver([(s, blocks_of(xs[s], 0, 12 + s)) for s in range(4)])
    got_own = [lv.d.process(own_pcm[:9 * B], want_precast=True)]             # the handle's own stream, between deliveries
    lv.d.reset_streams([3, 1])
    lv.forget([3, 1])
    lv.deliver([(s, blocks_of(xs[s], 12 + s, 20 + s)) for s in (2, 3, 0, 1)])
    got_batch = lv.d.process_batch(xs[0], [20, 16], want_precast=True, want_flags=True, want_noise=True)
    lv.deliver([(s, blocks_of(xs[s], 20 + s, 33)) for s in range(4)])
    got_own.append(lv.d.process(own_pcm[9 * B:], want_precast=True))
    lv.check(mode, what="listed streams start again, the others continue")
    assert lv.seen(0) == 33 and lv.seen(1) == 33 - 13
    for g, w in zip(got_own, want_own):
        assert np.array_equal(g[0], w[0]) and same_bits(g[1], w[1]), "the handle's own stream"
    for g, w in zip(got_batch, want_batch):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), "a batch call between deliveries"
    lv.d.reset_streams()                                                     # NULL: all
    lv.forget(range(4))
    noise, seen = lv.d.streams_state(range(4))
    assert not noise.any() and not seen.any()
    lv.deliver([(s, blocks_of(xs[s], 3, 17)) for s in (1, 0, 3)])
    lv.check(mode, what="after the reset of all")
    lv.close()


def test_the_python_entry_on_both_paths(eng):
    """Denoiser.process_streams: torch CUDA and numpy inputs give the same stream"""
    import torch
    x = speechlike(70, 20)
    y_i, y_f, y_flags, y_noise, _ = yardstick(eng, 1, x)
    for dev in (False, True):
        d = eng.denoiser(1)
        d.open_streams(3, 16)
        got_i, got_f, fl = [], [], []
        a = 0
        for n in (2, 5, 0, 13):
            pcm = np.concatenate([blocks_of(x, a, a + n), np.full(6, 32767, np.int16)])
            o, p, f, e = d.process_streams(torch.from_numpy(pcm).cuda() if dev else pcm, [2], [n], want_precast=True,
                                           want_flags=True)
            if dev:
                torch.cuda.synchronize()
                o, p, f, e = (t.cpu().numpy() for t in (o, p, f, e))
            got_i.append(o[:int(e[0]) * B])
            got_f.append(p[:int(e[0]) * B])
            fl.append(f)
            assert not o[int(e[0]) * B:].any() and not p[int(e[0]) * B:].any()
            a += n
        assert np.array_equal(np.concatenate(got_i), y_i) and same_bits(np.concatenate(got_f), y_f)
        assert np.array_equal(np.concatenate(fl), y_flags)
        assert same_bits(d.streams_state([2])[0][0], y_noise)
        d.close()


# ---- 6. errors -----------------------------------------------------------------------------------------------------------
def test_errors(eng):
    from jeicyboodsp_amd._lib import EINVAL
    L = lib()
    x = speechlike(80, 12)
    i64 = lambda *v: np.array(v, np.int64)       # noqa: E731

    def host(d, pcm, ids, first, blocks, n_samples=None):
        out = np.zeros(max(pcm.size, 1), np.int16)
        a_ids, a_first, a_blocks = i64(*ids), i64(*first), i64(*blocks)      # alive across the call
        return L.jdsp_denoise_streams(d._h, vp(pcm), pcm.size if n_samples is None else n_samples, vp(a_ids), vp(a_first),
                                      vp(a_blocks), len(ids), vp(out), None, None, None)

    def refused(rc, word):
        text = L.jdsp_last_error(eng._h).decode()
        assert rc == EINVAL and word in text, (rc, text)

    d = eng.denoiser(0)
    refused(host(d, x, [0], [0], [0, 2]), "jdsp_denoise_streams_reserve")                    # before reserve
    refused(L.jdsp_denoise_streams_dev(d._h, None, None, None, None, 1, 1, None, None, None, None), "reserve")
    refused(L.jdsp_denoise_streams_reset_dev(d._h, None, 0), "reserve")
    refused(L.jdsp_denoise_streams_state(d._h, vp(i64(0)), 1, None, None), "reserve")
    small = eng.denoiser(0, n_fft=512, hop=256)
    refused(L.jdsp_denoise_streams_reserve(small._h, 2, 8), "(1024, 512)")
    refused(host(small, x, [0], [0], [0, 2]), "(1024, 512)")
    refused(L.jdsp_denoise_streams_dev(small._h, None, None, None, None, 1, 1, None, None, None, None), "(1024, 512)")
    refused(L.jdsp_denoise_streams_reset_dev(small._h, None, 0), "(1024, 512)")
    refused(L.jdsp_denoise_streams_state(small._h, vp(i64(0)), 1, None, None), "(1024, 512)")
    small.close()
    d.close()

    lv = Live(eng, 0, 3, 8)
    lv.deliver([(0, blocks_of(x, 0, 4)), (2, blocks_of(x, 0, 3))])
    before = lv.d.streams_state([0, 1, 2])
    d = lv.d
    refused(host(d, x, [1, 1], [0, 1024], [0, 2, 4]), "twice")                              # a duplicate id
    refused(host(d, x, [3], [0], [0, 2]), "outside")                                        # an id out of range
    refused(host(d, x, [-1], [0], [0, 2]), "outside")
    refused(host(d, x, [0, 1, 2, 0], [0, 512, 1024, 1536], [0, 1, 2, 3, 4]), "more chunks")  # n_chunks > n_streams
    refused(host(d, x, [0, 1], [1024, 0], [0, 2, 4]), "ascend")                             # unsorted sample_first
    refused(host(d, x, [0], [1], [0, 2]), "even")                                           # odd sample_first
    refused(host(d, x, [0], [0], [0, 2], n_samples=1023), "past n_samples")                 # a span past n_samples
    refused(host(d, x, [0], [0], [0, 9]), "more blocks")                                    # more blocks than reserved
    refused(host(d, x, [0], [0], [1, 2]), "[0] must be 0")
    refused(host(d, x, [0, 1], [0, 2048], [0, 4, 2]), "decrease")
    # the scalars of the device entry
    refused(L.jdsp_denoise_streams_dev(d._h, None, None, None, None, 4, 4, None, None, None, None), "more chunks")
    refused(L.jdsp_denoise_streams_dev(d._h, None, None, None, None, 2, 9, None, None, None, None), "more blocks")
    refused(L.jdsp_denoise_streams_dev(d._h, None, None, None, None, -1, 2, None, None, None, None), "< 0")
    refused(L.jdsp_denoise_streams_dev(d._h, None, None, None, None, 1, 2, None, None, None, None), "NULL")
    refused(L.jdsp_denoise_streams_dev(d._h, C.c_void_p(8), None, None, None, 1, 2, None, None, None, None), "aligned")
    refused(L.jdsp_denoise_streams_reset_dev(d._h, C.c_void_p(16), 4), "n_ids")
    after = lv.d.streams_state([0, 1, 2])
    assert same_bits(before[0], after[0]) and np.array_equal(before[1], after[1])
    lv.deliver([(2, blocks_of(x, 3, 11))])
    lv.deliver([(0, blocks_of(x, 4, 12))])
    lv.deliver([(2, blocks_of(x, 11, 12))])
    lv.check(0, what="the refused calls left every stream as it was")
    lv.close()
