"""Live reverberation streams on the device (jdsp_reverb_streams*, include/jdsp.h "live reverberation streams"): every
stream of reverb_streams_cases under every cut pattern gives ONE set of bytes, int16 and float32, which is what
jdsp_reverb_batch writes for the stream as one utterance on the same handle; those bytes hold both bars against the FP64
direct convolution and the int16 rules; a switched stream's chunks are the batch's of (all blocks so far, ir_c, gain_c),
sliced; the company a stream keeps (ids, order, n_streams, neighbours, gaps) changes nothing; sentinels outside the spans
survive; NULL outputs advance the state; the state readback, the reset, the host entry, the batch entry in between, and
every error the header names.

Figures printed here (pytest -s) are recorded in profiles/r30_reverb_streams.txt."""
import ctypes as C

import numpy as np
import pytest

import reverb_cases as K
import reverb_streams_cases as S

pytestmark = pytest.mark.gpu
B = K.B
SENT_I = np.int16(0x5A5A)
SENT_F = np.float32(-7.25e11)
N_STREAMS = 1000
EINVAL = -1


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def handles(eng):
    """one handle per bank, made on first use and shared"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = eng.reverb(K.banks()[name])
        return made[name]
    yield get
    for h in made.values():
        h.close()


def vp(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def ids_of(n, n_streams, seed):
    """n distinct ids, sparse and unordered, the first, 7 and the last among them"""
    rng = np.random.default_rng(seed)
    rest = rng.choice(np.arange(8, n_streams - 1), size=max(n - 3, 0), replace=False).tolist()
    ids = np.array(([0, 7, n_streams - 1] + rest)[:n], np.int64)
    return ids[rng.permutation(n)]


def batch_bytes(rv, xs, ir, gain):
    """[(int16, float32)] of the utterances xs through the batch entry on the device"""
    import torch
    pcm, first, bf = K.pack(xs)
    a, b = rv.process_batch(torch.from_numpy(pcm).cuda(), first, bf, np.asarray(ir, np.int32), np.asarray(gain, np.float32),
                            want_f32=True)
    torch.cuda.synchronize()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return [(a[s:s + x.size].copy(), b[s:s + x.size].copy()) for x, s in zip(xs, first)]


def deliver(rv, entry, pcm, ids, counts, first, ir, gain, null=False):
    """one call; (int16, float32) numpy of pcm's length, or None with both outputs NULL (the device entry)"""
    import torch
    from jeicyboodsp_amd.engine import L
    if entry == "host":
        return rv.process_streams(pcm, ids, counts, ir, gain, chunk_sample_first=first, want_f32=True)
    n = pcm.size
    t = torch.from_numpy(np.ascontiguousarray(pcm)).cuda()
    if null:
        bf = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in
             (np.asarray(ids, np.int64), np.asarray(first, np.int64), bf, np.asarray(ir, np.int32), np.asarray(gain, np.float32))]
        rv.eng._use_torch_stream()
        rc = L.jdsp_reverb_streams_dev(rv._h, vp(t), vp(d[0]), vp(d[1]), vp(d[2]), vp(d[3]), vp(d[4]), len(ids), int(bf[-1]),
                                       None, None)
        assert rc == 0, L.jdsp_last_error(rv.eng._h).decode()
        torch.cuda.synchronize()
        return None
    o16 = torch.full((max(n, 1),), int(SENT_I), dtype=torch.int16, device="cuda")
    o32 = torch.full((max(n, 1),), float(SENT_F), dtype=torch.float32, device="cuda")
    a, b = rv.process_streams(t, ids, counts, ir, gain, chunk_sample_first=first, want_f32=True, out=o16, out_f32=o32)
    torch.cuda.synchronize()
    return a.cpu().numpy(), b.cpu().numpy()


def play(rv, name, ks, pattern_of, ids, seed, entry="dev", null_calls=(), check_state=False, between=None):
    """The streams ks of the bank, each under its pattern, delivered side by side to fresh live streams ids[k].
    Returns (int16 per stream, float32 per stream, the chunks per stream as (first, blocks, ir, gain, written))."""
    strs = [S.streams(name)[k] for k in ks]
    calls = S.deliveries(strs, rv.n_part, pattern_of, seed)
    g16 = [np.zeros(s.x.size, np.int16) for s in strs]
    g32 = [np.zeros(s.x.size, np.float32) for s in strs]
    log = [[] for _ in strs]
    seen = [0] * len(strs)
    rv.reset_streams()
    for t, chunks in enumerate(calls):
        gaps = [(0, 2, 768, 6, 0, 130)[(i + t + seed) % 6] for i in range(len(chunks))]
        pcm, first, counts = S.pack_call(strs, chunks, gaps, fill=32767, tail=2 * ((t + seed) % 3))
        null = t in null_calls
        res = deliver(rv, entry, pcm, [ids[c.stream] for c in chunks], counts, first, [c.ir for c in chunks],
                      [c.gain for c in chunks], null)
        keep = np.ones(pcm.size, bool)
        for c, a in zip(chunks, first):
            a = int(a)
            keep[a:a + c.blocks * B] = False
            seen[c.stream] += c.blocks
            if c.blocks:
                log[c.stream].append((c.first, c.blocks, c.ir, c.gain, not null))
            if not null:
                g16[c.stream][c.first * B:(c.first + c.blocks) * B] = res[0][a:a + c.blocks * B]
                g32[c.stream][c.first * B:(c.first + c.blocks) * B] = res[1][a:a + c.blocks * B]
        if not null and entry == "dev":
            assert np.all(res[0][:pcm.size][keep] == SENT_I), ("int16 written outside the spans", name, t)
            assert np.all(res[1][:pcm.size][keep].view(np.int32) == SENT_F.view(np.int32)), ("float32 outside", name, t)
        if not null and entry == "host":
            assert not res[0][keep].any() and not res[1][keep].any(), ("not zero outside the spans", name, t)
        if check_state:
            got_seen, got_last = rv.streams_state(ids[:len(strs)])
            assert got_seen.tolist() == seen, (name, t)
            for k, s in enumerate(strs):
                want = s.x[(seen[k] - 1) * B:seen[k] * B] if seen[k] else np.zeros(B, np.int16)
                assert np.array_equal(got_last[k], want), (name, t, k)
        if between:
            between(t)
    return g16, g32, log


def rotated(r, n):
    return [S.PATTERNS[(k + r) % len(S.PATTERNS)] for k in range(n)]


@pytest.fixture(scope="module")
def base(handles):
    """name -> the batch's bytes on the same handle: per constant stream the whole stream as one utterance, per
    switched stream and chunk the utterance "all blocks so far" with the chunk's pair; computed once per bank"""
    made = {}

    def get(name):
        if name in made:
            return made[name]
        rv = handles(name)
        strs = S.streams(name)
        const = [k for k, s in enumerate(strs) if s.cuts is None]
        whole = dict(zip(const, batch_bytes(rv, [strs[k].x for k in const], [strs[k].ir for k in const],
                                            [strs[k].gain for k in const])))
        pref = {}
        for k, s in enumerate(strs):
            if s.cuts is None:
                continue
            ends = np.cumsum(s.cuts)
            outs = batch_bytes(rv, [s.x[:e * B] for e in ends], s.ir, s.gain)
            for e, c, (a, b) in zip(ends, s.cuts, outs):
                pref[(k, int(e - c))] = (a[(e - c) * B:], b[(e - c) * B:])
        made[name] = (whole, pref)
        return made[name]
    return get


def check_against_batch(name, ks, g16, g32, log, base_of):
    """every written chunk of every stream equals the batch's bytes"""
    whole, pref = base_of
    strs = S.streams(name)
    for j, k in enumerate(ks):
        for first, blocks, ir, gain, written in log[j]:
            if not written:
                continue
            sl = slice(first * B, (first + blocks) * B)
            w16, w32 = (whole[k][0][sl], whole[k][1][sl]) if strs[k].cuts is None else pref[(k, first)]
            what = (name, k, strs[k].family, first, blocks, ir, gain)
            assert g32[j][sl].tobytes() == w32.tobytes(), ("float32 differs from the batch's", what)
            assert g16[j][sl].tobytes() == w16.tobytes(), ("int16 differs from the batch's", what)


# ---- one set of bytes, the batch's, within the bars -------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.BANKS)
def test_every_stream_under_every_pattern_gives_the_batchs_bytes_within_the_bars(handles, base, name):
    rv = handles(name)
    strs = S.streams(name)
    n = len(strs)
    ks = list(range(n))
    cap = sum(s.x.size // B for s in strs)
    worst = [0.0, 0.0]
    first_run = None
    for r in range(len(S.PATTERNS)):
        n_streams = N_STREAMS if r % 2 == 0 else 257           # another n_streams, other ids, another order, other gaps
        rv.open_streams(n_streams, cap)
        g16, g32, log = play(rv, name, ks, rotated(r, n), ids_of(n, n_streams, 40 + r), r, check_state=r in (0, 3))
        check_against_batch(name, ks, g16, g32, log, base(name))
        if first_run is None:
            first_run = (g16, g32)
        for k in ks:                                           # one set of bytes, whatever the pattern
            assert g16[k].tobytes() == first_run[0][k].tobytes() and g32[k].tobytes() == first_run[1][k].tobytes(), (name, r, k)
    g16, g32 = first_run
    for k, s in enumerate(strs):
        if s.cuts is None:
            u = S.whole_oracle(name, k)
            g, loc = K.ratios_of(g32[k], u)
            own, far = K.int16_rules(g16[k], g32[k], u)
            what = (name, k, s.family, s.ir, s.gain)
            assert g <= 1.0 and loc <= 1.0, (what, g, loc)
            assert own == 0 and far == 0, (what, own, far)
            if K.must_be_zero(u):
                assert not g32[k].any() and not g16[k].any(), what
            worst = [max(worst[0], g), max(worst[1], loc)]
            continue
        at = 0
        for c, ir, gain in zip(s.cuts, s.ir, s.gain):
            want = S.chunk_oracle(name, k, at, c, ir, gain)
            sl = slice(at * B, (at + c) * B)
            what = (name, k, s.family, at, c, ir, gain)
            if want.zero or gain == 0.0:                       # gain 0: exact zeros, either sign
                assert not g32[k][sl].any() and not g16[k][sl].any(), what
            g, loc = S.ratios(g32[k][sl], want)
            assert g <= 1.0 and loc <= 1.0, (what, g, loc)
            u = K.Utt(None, ir, gain, "", want.w, want.global_bar, want.local_bar)
            assert K.int16_rules(g16[k][sl], g32[k][sl], u) == (0, 0), what
            worst = [max(worst[0], g), max(worst[1], loc)]
            at += c
    print("\n  %-10s P = %2d, %2d streams x %d patterns, %d blocks: worst fraction of the global bar %.4f, of the local "
          "bar %.4f" % (name, rv.n_part, n, len(S.PATTERNS), cap, worst[0], worst[1]))


@pytest.mark.parametrize("name", ["taps513", "rir7169"])
def test_a_stream_does_not_depend_on_its_company(handles, base, name):
    """fewer streams, alone, and with neighbours on other responses and gains: the same bytes"""
    rv = handles(name)
    strs = S.streams(name)
    rv.open_streams(64, sum(s.x.size // B for s in strs))
    for ks in ([0, 6, 9, 10], [6], [10, 3]):
        g16, g32, log = play(rv, name, ks, rotated(2, len(ks)), ids_of(len(ks), 64, 50 + len(ks)), 9)
        check_against_batch(name, ks, g16, g32, log, base(name))


# ---- NULL outputs, the state, the reset ---------------------------------------------------------------------------------------
def test_both_outputs_null_advance_the_state(handles, base):
    name = "taps1025"
    rv = handles(name)
    ks = [0, 4, 6, 9]
    rv.open_streams(N_STREAMS, 64)
    ids = ids_of(len(ks), N_STREAMS, 60)
    g16, g32, log = play(rv, name, ks, ["odd", "single", "around_p", "own"], ids, 3, null_calls=(1, 2), check_state=True)
    assert any(not w for chunks in log for *_, w in chunks) and any(w for chunks in log for c in chunks[2:] for *_, w in [c])
    check_against_batch(name, ks, g16, g32, log, base(name))   # the chunks behind the silent calls are what they would be


def test_reset_of_a_subset_and_of_all(handles, base):
    import torch
    name = "taps1025"
    rv = handles(name)
    strs = S.streams(name)
    P = rv.n_part
    whole, _ = base(name)
    rv.open_streams(N_STREAMS, 64)
    ids = np.array([999, 3, 500], np.int64)
    ks = [0, 2, 6]

    def call(first_block, blocks, which=(0, 1, 2)):
        xs = [strs[ks[j]].x[first_block * B:(first_block + blocks) * B] for j in which]
        pcm, first, bf = K.pack(xs, [2] * len(xs), fill=-32768)
        res = deliver(rv, "dev", pcm, ids[list(which)], np.diff(bf), first, [strs[ks[j]].ir for j in which],
                      [strs[ks[j]].gain for j in which])
        return [(res[0][a:a + blocks * B], res[1][a:a + blocks * B]) for a in first]

    rv.reset_streams()
    call(0, P + 1)
    rv.reset_streams([999, 500])                               # streams 0 and 2 of the three
    seen, last = rv.streams_state(ids)
    assert seen.tolist() == [0, P + 1, 0] and not last[0].any() and not last[2].any()
    assert np.array_equal(last[1], strs[ks[1]].x[P * B:(P + 1) * B])
    got = call(P + 1, 3)
    fresh = batch_bytes(rv, [strs[ks[j]].x[(P + 1) * B:(P + 4) * B] for j in (0, 2)], [strs[ks[j]].ir for j in (0, 2)],
                        [strs[ks[j]].gain for j in (0, 2)])
    sl = slice((P + 1) * B, (P + 4) * B)
    for j, f in zip((0, 2), fresh):                            # a fresh stream's bytes: the chunk as an utterance
        assert got[j][0].tobytes() == f[0].tobytes() and got[j][1].tobytes() == f[1].tobytes(), j
        assert got[j][1].tobytes() != whole[ks[j]][1][sl].tobytes()
    assert got[1][0].tobytes() == whole[ks[1]][0][sl].tobytes() and got[1][1].tobytes() == whole[ks[1]][1][sl].tobytes()
    rv.reset_streams()                                         # NULL: all
    seen, last = rv.streams_state(ids)
    assert seen.tolist() == [0, 0, 0] and not last.any()
    got = call(0, 2)
    for j in range(3):
        assert got[j][1].tobytes() == whole[ks[j]][1][:2 * B].tobytes()
    torch.cuda.synchronize()


# ---- the host entry; the batch entry in between -----------------------------------------------------------------------------------
def test_the_host_entry_gives_the_device_entrys_bytes_and_zeros_outside_the_spans(handles, base):
    name = "taps513"
    rv = handles(name)
    strs = S.streams(name)
    ks = list(range(len(strs)))
    rv.open_streams(N_STREAMS, sum(s.x.size // B for s in strs))
    g16, g32, log = play(rv, name, ks, rotated(4, len(ks)), ids_of(len(ks), N_STREAMS, 70), 5, entry="host", check_state=True)
    check_against_batch(name, ks, g16, g32, log, base(name))   # which are the device entry's (the test above)


def test_the_batch_entry_in_between_changes_neither(handles, base):
    name = "dense7680"
    rv = handles(name)
    strs = S.streams(name)
    whole, _ = base(name)
    ks = [0, 6, 8, 10]
    rv.open_streams(N_STREAMS, sum(strs[k].x.size // B for k in ks))
    n_between = [0]

    def between(t):
        if t % 5 == 0:
            a, b = batch_bytes(rv, [strs[0].x, strs[6].x[:3 * B]], [strs[0].ir, strs[6].ir], [strs[0].gain, strs[6].gain])[0]
            assert a.tobytes() == whole[0][0].tobytes() and b.tobytes() == whole[0][1].tobytes(), t
            n_between[0] += 1

    g16, g32, log = play(rv, name, ks, ["single", "odd", "one", "own"], ids_of(len(ks), N_STREAMS, 80), 6, between=between)
    assert n_between[0] > 3
    check_against_batch(name, ks, g16, g32, log, base(name))


# ---- errors ------------------------------------------------------------------------------------------------------------------
def _err(eng):
    from jeicyboodsp_amd.engine import L
    return L.jdsp_last_error(eng._h).decode()


def test_errors_of_the_live_entries(eng):
    import torch
    import jeicyboodsp_amd
    from jeicyboodsp_amd.engine import L
    rv = eng.reverb(K.banks()["taps513"])
    x = K.utterance("white", 5, 95)
    pcm_h, first_h, bf_h = K.pack([x[:2 * B], x[2 * B:]], [0, 4])
    ids_h = np.array([2, 0], np.int64)
    pcm = torch.from_numpy(pcm_h).cuda()
    ids, first, bf = (torch.from_numpy(a).cuda() for a in (ids_h, first_h, bf_h))
    ir = torch.zeros(2, dtype=torch.int32, device="cuda")
    gain = torch.ones(2, dtype=torch.float32, device="cuda")
    o16 = torch.zeros(pcm_h.size + 8, dtype=torch.int16, device="cuda")
    o32 = torch.zeros(pcm_h.size + 8, dtype=torch.float32, device="cuda")
    eng._use_torch_stream()

    def dev(n_chunks=2, n_total=5, p=None, idp=None, sf=None, bfp=None, irp=None, gp=None, a=None, b=None):
        return L.jdsp_reverb_streams_dev(rv._h, p or vp(pcm), idp or vp(ids), sf or vp(first), bfp or vp(bf), irp or vp(ir),
                                         gp or vp(gain), n_chunks, n_total, a or vp(o16), b or vp(o32))

    seen_h = np.zeros(1, np.int64)
    # any entry before the reservation
    assert dev() == EINVAL and "jdsp_reverb_streams_reserve" in _err(eng)
    assert dev(n_chunks=0, n_total=0) == EINVAL and "jdsp_reverb_streams_reserve" in _err(eng)
    assert L.jdsp_reverb_streams_reset_dev(rv._h, None, 0) == EINVAL and "jdsp_reverb_streams_reserve" in _err(eng)
    assert L.jdsp_reverb_streams_state(rv._h, ids_h.ctypes.data_as(C.c_void_p), 1, seen_h.ctypes.data_as(C.c_void_p),
                                       None) == EINVAL and "jdsp_reverb_streams_reserve" in _err(eng)
    with pytest.raises(jeicyboodsp_amd.JdspError) as e:
        rv.process_streams(pcm_h, ids_h, np.diff(bf_h), [0, 0], chunk_sample_first=first_h)
    assert e.value.code == EINVAL and "jdsp_reverb_streams_reserve" in str(e.value)
    for bad in ((0, 1), (1, -1), (2 ** 30, 1), (1, 2 ** 30)):
        assert L.jdsp_reverb_streams_reserve(rv._h, *bad) == EINVAL and "jdsp_reverb_streams_reserve" in _err(eng)
    rv.open_streams(3, 5)
    assert dev() == 0
    state0 = [a.copy() for a in rv.streams_state([0, 1, 2])]
    assert state0[0].tolist() == [3, 0, 2]
    # beyond the reservation, more chunks than streams, negative counts
    assert dev(n_total=6) == EINVAL and "jdsp_reverb_streams_reserve sized" in _err(eng)
    assert dev(n_chunks=4) == EINVAL and "more chunks than live streams" in _err(eng)
    assert dev(n_chunks=-1) == EINVAL and dev(n_total=-1) == EINVAL
    # misaligned pointers
    for kw in (dict(p=vp(pcm, 2)), dict(a=vp(o16, 2)), dict(b=vp(o32, 4)), dict(idp=vp(ids, 4)), dict(sf=vp(first, 4)),
               dict(bfp=vp(bf, 4)), dict(irp=vp(ir, 2)), dict(gp=vp(gain, 2))):
        assert dev(**kw) == EINVAL and "aligned" in _err(eng), kw
    assert L.jdsp_reverb_streams_reset_dev(rv._h, vp(ids, 4), 1) == EINVAL and "aligned" in _err(eng)
    assert L.jdsp_reverb_streams_reset_dev(rv._h, vp(ids), 4) == EINVAL and "n_ids" in _err(eng)
    # NULL inputs with work to do
    assert L.jdsp_reverb_streams_dev(rv._h, None, vp(ids), vp(first), vp(bf), vp(ir), None, 2, 5, vp(o16), None) == EINVAL
    assert L.jdsp_reverb_streams_dev(rv._h, vp(pcm), None, vp(first), vp(bf), vp(ir), None, 2, 5, vp(o16), None) == EINVAL
    assert "NULL" in _err(eng)
    # nothing to do is no error and changes nothing
    assert dev(n_chunks=0, n_total=0) == 0 and dev(n_chunks=2, n_total=0) == 0
    torch.cuda.synchronize()

    # the host entry: every violation is EINVAL with a text, and the state is as it was
    def host(ids=ids_h, first=first_h, bf=bf_h, ir=(0, 2), gain=(1.0, 1.0), pcm=pcm_h):
        with pytest.raises(jeicyboodsp_amd.JdspError) as e:
            rv.process_streams(pcm, ids, np.diff(bf), ir, gain, chunk_sample_first=first)
        assert e.value.code == EINVAL and "jdsp_reverb_streams" in str(e.value)
        now = rv.streams_state([0, 1, 2])
        assert np.array_equal(now[0], state0[0]) and np.array_equal(now[1], state0[1])
        return str(e.value)
    assert "occurs twice" in host(ids=np.array([1, 1]))
    assert "outside [0, n_streams)" in host(ids=np.array([0, 3])) and "outside [0, n_streams)" in host(ids=np.array([-1, 0]))
    assert "outside [0, n_irs)" in host(ir=(0, 3)) and "outside [0, n_irs)" in host(ir=(-1, 0))
    assert "finite" in host(gain=(1.0, np.nan)) and "finite" in host(gain=(np.inf, 1.0))
    assert "overlap" in host(first=np.array([0, 512], np.int64))
    assert "even" in host(first=first_h + 1)
    assert "past n_samples" in host(pcm=pcm_h[:-2])
    assert "sized" in host(first=np.array([0, 3 * B + 4], np.int64), bf=np.array([0, 3, 6], np.int64),
                           pcm=np.zeros(6 * B + 4, np.int16))
    with pytest.raises(jeicyboodsp_amd.JdspError):                          # more chunks than streams
        rv.process_streams(np.zeros(4 * B, np.int16), [0, 1, 2, 2], [1, 1, 1, 1], [0, 0, 0, 0])
    o = rv.process_streams(pcm_h, ids_h, np.diff(bf_h), (0, 2), (1.0, 1.0), chunk_sample_first=first_h)
    assert o.size == pcm_h.size and rv.streams_state([0, 1, 2])[0].tolist() == [6, 0, 4]
    rv.close()
