"""Live binaural rendering (jdsp_binaural_*, include/jdsp.h "binaural rendering") on the GPU against the FP64
reference of tests/binaural_ref.py: the four guarantees of the header (accuracy, cuts, independence, exact silence),
the fades, the state rule, a cross-check against the reference-pinned convolver, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import binaural_ref as R

pytestmark = pytest.mark.gpu

BLOCK = 512


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def layout(blocks, chunks):
    from jeicyboodsp_amd.sharding import binaural_layout
    return binaural_layout(blocks, chunks)


def as_np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def render(h, pcm, args, device, plane=None):
    """one delivery through the host entry (numpy) or the device entry (torch): (int16 [2, plane], float32 [2, plane])"""
    if device:
        import torch
        pcm = torch.from_numpy(np.ascontiguousarray(pcm)).cuda()
    o16, o32 = h.render(pcm, *args, plane=plane, want_i16=True, want_f32=True)
    if device:
        import torch
        torch.cuda.synchronize()
    return as_np(o16), as_np(o32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def sources(seed, n_chunks, n_samples_each):
    """per chunk its PCM: noise, every fourth a voiced tone"""
    return [R.make_pcm(seed + 7 * c, n_samples_each, voiced=(c % 4 == 3)) for c in range(n_chunks)]


# ---- guarantee 1: accuracy ------------------------------------------------------------------------------------------
FIVE = ([0, 1, 2, 8, 17], [[1, 2, 3, 2, 1], [3, 1, 2, 1, 2], [2, 3, 1, 3, 1], [1, 1, 1, 2, 3]])
ONE = ([8], [[2], [1], [3], [1]])


@pytest.mark.parametrize("n_taps", [1, 2, 512, 513])
@pytest.mark.parametrize("shape", [ONE, FIVE], ids=["one_mix", "five_mixes"])
def test_accuracy_over_four_deliveries(eng, n_taps, shape):
    """chunks per mix 0, 1, 2, 8, 17; B of 1, 2, 3 (the same wave reads and writes state, a first and a last wave, a
    middle one); delivery 1 changes every (dir, gain), delivery 2 some chunks only (dir alone, gain alone, both),
    delivery 3 none; sparse ids in n_streams = 40; the host entry and the device entry in turn"""
    chunks, blocks_of = shape
    n_dirs, n_streams, n_chunks = 7, 40, sum(chunks)
    bank = R.make_bank(100 + n_taps, n_dirs, n_taps)
    h = eng.binaural(bank)
    h.open_streams(n_streams)
    ref = R.RefBinaural(bank, n_streams)
    rng = np.random.default_rng(n_taps + n_chunks)
    ids = rng.permutation(n_streams)[:n_chunks]
    src = sources(n_taps, n_chunks, BLOCK * sum(max(b) for b in blocks_of))
    at = np.zeros(n_chunks, np.int64)
    dirs = rng.integers(0, n_dirs, n_chunks)
    gains = rng.uniform(0.1, 2.0, n_chunks).astype(np.float32)
    worst = 0.0
    for k, blocks in enumerate(blocks_of):
        if k == 1:
            dirs = (dirs + 1 + rng.integers(0, n_dirs - 1, n_chunks)) % n_dirs
            gains = rng.uniform(0.1, 2.0, n_chunks).astype(np.float32)
        if k == 2:
            sel = np.arange(n_chunks)
            dirs = np.where(sel % 3 == 0, (dirs + 1) % n_dirs, dirs)
            gains = np.where(sel % 3 == 1, np.float32(0.5) * gains + np.float32(0.1), gains).astype(np.float32)
            both = sel % 5 == 4
            dirs = np.where(both, (dirs + 2) % n_dirs, dirs)
            gains = np.where(both, np.float32(2.0) - gains * np.float32(0.5), gains).astype(np.float32)
        sf, cf, bf, mix, n = layout(blocks, chunks)
        pcm = np.zeros(n, np.int16)
        for c in range(n_chunks):
            nb = blocks[mix[c]]
            pcm[sf[c]:sf[c] + BLOCK * nb] = src[c][BLOCK * at[c]:BLOCK * (at[c] + nb)]
            at[c] += nb
        args = (ids, sf, dirs, gains, cf, bf)
        want, bar = ref.render(pcm, *args)
        o16, o32 = render(h, pcm, args, device=bool(k & 1))
        w = R.check_block_outputs(o16, o32, want, bar, (n_taps, chunks, k))
        worst = max(worst, w)
        print("binaural accuracy taps %d chunks %s delivery %d: worst error / bar %.3f" % (n_taps, chunks, k, w))
        if chunks[0] == 0:                                    # the mix without a chunk: its blocks are zeros
            assert not o32[:, :BLOCK * blocks[0]].any() and not o16[:, :BLOCK * blocks[0]].any()
    hist, d, g, st = h.streams_state(ids)
    assert np.array_equal(hist, ref.hist[ids]) and np.array_equal(d, ref.dir[ids]) and same_bits(g, ref.gain[ids])
    assert np.all(st == 1)
    h.close()


# ---- guarantee 2: cuts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "dev"])
def test_cuts_give_the_same_bits(eng, device):
    """one block at (d0, g0), six blocks at (d1, g1) cut as 6, 3+3, 2+2+2, 1x6 and 1+5, one block at (d2, g2): the two
    changes stand at boundaries every cut has; two mixes, of three sources and of one"""
    bank = R.make_bank(21, 5, 400)
    chunks, n_chunks = [3, 1], 4
    src = sources(31, n_chunks, BLOCK * 8)
    ids = np.array([5, 0, 3, 2])
    d = [np.array([0, 1, 2, 3]), np.array([1, 1, 4, 0]), np.array([2, 1, 4, 0])]
    g = [np.float32([1.0, 0.5, 1.5, 0.8]), np.float32([0.7, 0.5, 1.5, 1.9]), np.float32([0.7, 0.25, 1.5, 1.9])]
    h = eng.binaural(bank)
    h.open_streams(6)
    ref = R.RefBinaural(bank, 6)

    def run(cuts, check):
        h.reset_streams()
        ref.reset()
        plan = [(1, 0)] + [(n, 1) for n in cuts] + [(1, 2)]
        at, i16, f32 = 0, [], []
        for nb, which in plan:
            sf, cf, bf, mix, n = layout([nb, nb], chunks)
            pcm = np.concatenate([src[c][BLOCK * at:BLOCK * (at + nb)] for c in range(n_chunks)])
            args = (ids, sf, d[which], g[which], cf, bf)
            o16, o32 = render(h, pcm, args, device)
            if check:
                R.check_block_outputs(o16, o32, *ref.render(pcm, *args), what=("cut", cuts, at))
            # mix 0's blocks, then mix 1's: keep them apart so that every cut concatenates to the same layout
            i16.append((o16[:, :BLOCK * nb], o16[:, BLOCK * nb:]))
            f32.append((o32[:, :BLOCK * nb], o32[:, BLOCK * nb:]))
            at += nb
        cat = lambda parts: np.concatenate([np.concatenate([p[m] for p in parts], axis=1) for m in range(2)], axis=1)
        return cat(i16), cat(f32), h.streams_state(ids)

    whole = run([6], True)
    for cuts in ([3, 3], [2, 2, 2], [1] * 6, [1, 5]):
        got = run(cuts, False)
        assert np.array_equal(got[0], whole[0]), cuts
        assert same_bits(got[1], whole[1]), cuts
        assert all(same_bits(a, b) for a, b in zip(got[2], whole[2])), cuts
    h.close()


# ---- guarantee 3: independence, and the state rule -----------------------------------------------------------------
def test_a_mix_does_not_depend_on_its_place_ids_or_n_streams(eng):
    bank = R.make_bank(41, 4, 257)
    src = sources(51, 3, BLOCK * 4)
    others = sources(61, 9, BLOCK * 6)
    plan = [(2, [0, 1, 2], np.float32([1.0, 0.6, 1.4])), (2, [0, 3, 2], np.float32([1.0, 0.6, 0.9]))]   # delivery 1 fades two

    def alone():
        h = eng.binaural(bank)
        h.open_streams(3)
        outs = []
        for k, (nb, dirs, gains) in enumerate(plan):
            sf, cf, bf, _, _ = layout([nb], [3])
            pcm = np.concatenate([s[BLOCK * 2 * k:BLOCK * 2 * (k + 1)] for s in src])
            outs.append(render(h, pcm, ([0, 1, 2], sf, dirs, gains, cf, bf), True))
        h.close()
        return outs

    def last_of_five(order):
        h = eng.binaural(bank)
        h.open_streams(40)
        ids_x, outs = [30, 7, 19], []
        ids_o = [1, 2, 3, 4, 5, 6, 8, 9, 10]
        for k, (nb, dirs, gains) in enumerate(plan):
            blocks, chunks = [1, 3, 0, 2, nb], [2, 3, 1, 3, 3]
            sf, cf, bf, mix, n = layout(blocks, chunks)
            pcm = np.zeros(n, np.int16)
            for c in range(9):
                pcm[sf[c]:sf[c] + BLOCK * blocks[mix[c]]] = others[c][BLOCK * 3 * k:BLOCK * (3 * k + blocks[mix[c]])]
            for c in range(3):
                pcm[sf[9 + c]:sf[9 + c] + BLOCK * nb] = src[c][BLOCK * 2 * k:BLOCK * 2 * (k + 1)]
            args = [np.array(ids_o + ids_x), sf, np.array([1, 2, 3, 0, 1, 2, 3, 0, 1] + list(dirs)),
                    np.concatenate([np.float32([0.3] * 9), gains]), cf, bf]
            if order == "x_first":
                # the same five mixes, X in front: chunk and block axes rebuilt
                perm_m = [4, 0, 1, 2, 3]
                b2, c2 = [blocks[m] for m in perm_m], [chunks[m] for m in perm_m]
                cperm = np.concatenate([np.arange(cf[m], cf[m + 1]) for m in perm_m]).astype(np.int64)
                _, cf2, bf2, _, _ = layout(b2, c2)
                args = [args[0][cperm], sf[cperm], args[2][cperm], args[3][cperm], cf2, bf2]
                o16, o32 = render(h, pcm, args, True)
                outs.append((o16[:, :BLOCK * nb], o32[:, :BLOCK * nb]))
            else:
                o16, o32 = render(h, pcm, args, True)
                outs.append((o16[:, BLOCK * int(bf[4]):], o32[:, BLOCK * int(bf[4]):]))
        h.close()
        return outs

    a, b, c = alone(), last_of_five("x_last"), last_of_five("x_first")
    for k in range(2):
        for other in (b, c):
            assert np.array_equal(a[k][0], other[k][0]) and same_bits(a[k][1], other[k][1]), k


def test_chunk_order_matters_and_is_the_list_order(eng):
    """stated, not hidden: the sum is taken in list order, so another order of a mix's own chunks may give other bits,
    and each order meets the reference"""
    bank = R.make_bank(42, 3, 100)
    src = sources(52, 5, BLOCK)
    sf, cf, bf, _, _ = layout([1], [5])
    pcm = np.concatenate(src)
    h = eng.binaural(bank)
    h.open_streams(5)
    gains = np.float32([2.0, 0.1, 1.3, 0.7, 1.9])
    dirs = np.array([0, 1, 2, 0, 1])
    for perm in (np.arange(5), np.array([4, 2, 0, 3, 1])):
        h.reset_streams()
        ref = R.RefBinaural(bank, 5)
        args = (np.arange(5)[perm], sf[perm], dirs[perm], gains[perm], cf, bf)
        o16, o32 = render(h, pcm, args, True)
        R.check_block_outputs(o16, o32, *ref.render(pcm, *args), what=tuple(perm))
    h.close()


def test_two_streams_hear_one_span_and_absent_streams_stay(eng):
    bank = R.make_bank(43, 3, 64)
    pcm = np.concatenate([R.make_pcm(71, BLOCK * 2), R.make_pcm(72, BLOCK * 2, voiced=True)])
    h = eng.binaural(bank)
    h.open_streams(8)
    ref = R.RefBinaural(bank, 8)
    every = np.arange(8)
    # streams 6 and 1 in two mixes read the same span; stream 4 is in a mix of no blocks; the rest have no chunk
    args = (np.array([6, 4, 1]), np.array([0, 2048, 0]), np.array([2, 1, 2]), np.float32([0.9, 1.0, 0.9]),
            np.array([0, 1, 2, 3]), np.array([0, 2, 2, 4]))
    before = h.streams_state(every)
    o16, o32 = render(h, pcm, args, False)
    R.check_block_outputs(o16, o32, *ref.render(pcm, *args))
    assert np.array_equal(o16[:, :1024], o16[:, 1024:]) and same_bits(o32[:, :1024], o32[:, 1024:])
    after = h.streams_state(every)
    absent = np.array([0, 2, 3, 4, 5, 7])
    for x, y in zip(before, after):
        assert same_bits(x[absent], y[absent])
    hist, d, g, st = after
    for s in (6, 1):
        assert np.array_equal(hist[s], pcm[BLOCK:2 * BLOCK]) and d[s] == 2 and same_bits(g[s:s + 1], np.float32([0.9])) and st[s] == 1
    assert not st[absent].any()
    # a second delivery moves only stream 1; a reset of stream 6 makes it fresh, nothing else
    args2 = (np.array([1]), np.array([1024]), np.array([0]), np.float32([0.9]), np.array([0, 1]), np.array([0, 2]))
    o16, o32 = render(h, pcm, args2, True)
    R.check_block_outputs(o16, o32, *ref.render(pcm, *args2))
    h.reset_streams([6])
    hist, d, g, st = h.streams_state(every)
    assert st.tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and not hist[6].any() and d[1] == 0
    assert np.array_equal(hist[1], pcm[3 * BLOCK:4 * BLOCK])
    h.close()


# ---- fades, guarantee 4 --------------------------------------------------------------------------------------------
def test_fade_to_silence_then_exact_zeros(eng):
    bank = R.make_bank(44, 2, 513)
    pcm = R.make_pcm(73, BLOCK * 4)
    h = eng.binaural(bank)
    h.open_streams(1)
    ref = R.RefBinaural(bank, 1)
    one = lambda at, nb, d, gain: ([0], [BLOCK * at], [d], np.float32([gain]), [0, 1], [0, nb])
    for args, dev in ((one(0, 1, 0, 1.0), False), (one(1, 1, 0, 0.0), True)):
        o16, o32 = render(h, pcm, args, dev)
        want, bar = ref.render(pcm, *args)
        R.check_block_outputs(o16, o32, want, bar)
    assert np.abs(want[:, :64]).max() > 100 and np.abs(want[:, -1]).max() < 0.01 * np.abs(want).max()   # it did fade out
    # carried gain 0.0 and delivered gain 0.0: exact zeros, also while the direction moves (a faded block of zeros)
    for args in (one(2, 1, 0, 0.0), one(3, 1, 1, 0.0)):
        o16, o32 = render(h, pcm, args, True)
        assert not o16.any() and not o32.any()
    h.close()


def test_direction_change_then_plain_form_bit_for_bit(eng):
    """A moves 0 -> 1 between deliveries; B had direction 1 all along and the same history.  A's faded block meets the
    reference; from the block behind it on both are the plain form of the same samples: the same bits."""
    bank = R.make_bank(45, 2, 333)
    pcm = R.make_pcm(74, BLOCK * 4, voiced=True) // 2 + R.make_pcm(75, BLOCK * 4) // 2
    h = eng.binaural(bank)
    h.open_streams(2)
    ref = R.RefBinaural(bank, 2)
    # two single-source mixes over the same PCM: stream 0 is A, stream 1 is B
    plan = [(0, 1, [0, 1]), (1, 2, [1, 1]), (3, 1, [1, 1])]
    for at, nb, dirs in plan:
        args = ([0, 1], [BLOCK * at] * 2, dirs, np.float32([1.2, 1.2]), [0, 1, 2], [0, nb, 2 * nb])
        o16, o32 = render(h, pcm, args, True)
        want, bar = ref.render(pcm, *args)
        R.check_block_outputs(o16, o32, want, bar, what=at)
        a16, b16, a32, b32 = o16[:, :BLOCK * nb], o16[:, BLOCK * nb:], o32[:, :BLOCK * nb], o32[:, BLOCK * nb:]
        if at == 1:
            assert not np.array_equal(a32[:, :BLOCK], b32[:, :BLOCK])                 # the faded block differs ...
            assert np.abs(want[:, :BLOCK] - want[:, 2 * BLOCK:3 * BLOCK]).max() > 50
            assert np.array_equal(a16[:, BLOCK:], b16[:, BLOCK:]) and same_bits(a32[:, BLOCK:], b32[:, BLOCK:])
        if at == 3:
            assert np.array_equal(a16, b16) and same_bits(a32, b32)
    h.close()


# ---- the reference-pinned convolver ----------------------------------------------------------------------------------
def test_against_fastconv_1024(eng):
    """one source, gain 1, a constant direction, 513 taps: jdsp_fastconv (n_fft 1024, the same two filters) emits the
    same stream from its emitted block 1 on (its block 0 takes the stream's first block as silence).  Each side is
    within one bar of the truth, so they agree within two."""
    bank = R.make_bank(46, 3, 513)
    n_blocks = 6
    pcm = R.make_pcm(76, BLOCK * n_blocks)
    h = eng.binaural(bank)
    h.open_streams(1)
    ref = R.RefBinaural(bank, 1)
    args = ([0], [0], [2], np.float32([1.0]), [0, 1], [0, n_blocks])
    o16, o32 = render(h, pcm, args, True)
    want, bar = ref.render(pcm, *args)
    R.check_block_outputs(o16, o32, want, bar)
    fc = eng.fastconv(bank[2], 1024)
    assert fc.block == BLOCK and fc.hist_blocks == 1
    f16, f32 = fc.process(pcm, want_precast=True)
    assert f32.shape == (2, BLOCK * (n_blocks - 1))
    err = np.abs(f32[:, BLOCK:].astype(np.float64) - o32[:, 2 * BLOCK:]).reshape(2, n_blocks - 2, BLOCK).max(axis=(0, 2))
    print("binaural vs fastconv: worst difference / bar %.3f" % (err / (1e-5 * bar[2:])).max())
    assert np.all(err <= 2e-5 * bar[2:])
    assert np.abs(f16[:, BLOCK:].astype(np.int32) - o16[:, 2 * BLOCK:]).max() <= 1
    fc.close()
    h.close()


# ---- refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_every_stream_as_it_was(eng):
    from jeicyboodsp_amd._lib import EINVAL, JdspError
    from jeicyboodsp_amd.engine import L, _vp
    import torch
    bank = R.make_bank(47, 3, 16)
    for bad in (np.zeros((3, 2, 514)), np.zeros((0, 2, 4))):
        with pytest.raises(JdspError) as e:
            eng.binaural(bad)
        assert e.value.code == EINVAL and "jdsp_binaural_create" in str(e.value)
    h = eng.binaural(bank)
    assert L.jdsp_binaural_n_dirs(h._h) == 3 and h.block == 512
    pcm = R.make_pcm(77, BLOCK * 4)
    good = dict(ids=[1, 3], sf=[0, 1024], dirs=[0, 2], gains=np.float32([1.0, 0.5]), cf=[0, 1, 2], bf=[0, 2, 4])

    def call(**kw):
        a = dict(good, **kw)
        return h.render(a.get("pcm", pcm), a["ids"], a["sf"], a["dirs"], a["gains"], a["cf"], a["bf"], plane=a.get("plane"),
                        want_i16=True, want_f32=True)

    def refused(text, fn, *args, **kw):
        with pytest.raises(JdspError) as e:
            fn(*args, **kw)
        assert e.value.code == EINVAL and text in str(e.value), str(e.value)

    # before jdsp_binaural_streams_reserve: the stream entries refuse, with a text
    refused("jdsp_binaural_streams_reserve first", call)
    refused("jdsp_binaural_streams_reserve first", call, pcm=torch.from_numpy(pcm).cuda())
    refused("jdsp_binaural_streams_reserve first", h.reset_streams)
    refused("jdsp_binaural_streams_reserve first", h.streams_state, [0])
    refused("n_streams", h.open_streams, 0)
    h.open_streams(4)
    call()                                                       # a sound delivery: the streams now carry something
    torch.cuda.synchronize()
    every = np.arange(4)
    before = h.streams_state(every)
    refused("a stream id occurs twice", call, ids=[1, 1])
    refused("outside [0, n_streams)", call, ids=[1, 4])
    refused("outside [0, n_streams)", call, ids=[-1, 2])
    refused("more chunks than live streams", call, ids=[0, 1, 2, 3, 0], sf=[0] * 5, dirs=[0] * 5, gains=np.float32([1] * 5),
            cf=[0, 5, 5])
    refused("chunk_first[0] must be 0", call, cf=[1, 1, 2])
    refused("block_first[0] must be 0", call, bf=[1, 2, 4])
    refused("chunk_first must not decrease", call, cf=[0, 3, 2])
    refused("block_first must not decrease", call, bf=[0, 3, 2])
    refused("chunk_first[n_mixes] must be n_chunks", call, cf=[0, 1, 1])
    refused("a dir lies outside", call, dirs=[0, 3])
    refused("a dir lies outside", call, dirs=[-1, 0])
    refused("a gain is not finite", call, gains=np.float32([np.inf, 1]))
    refused("a gain is not finite", call, gains=np.float32([1, np.nan]))
    refused("sample_first entries must be even", call, sf=[0, 1023])
    refused("sample_first entries must be even", call, sf=[-2, 1024])
    refused("ends past n_samples", call, sf=[0, 1026])
    refused("plane must be even", call, plane=2049)
    refused("do not fit in plane", call, plane=2046)
    refused("outside [0, n_streams)", h.streams_state, [4])
    # the device entry's own checks: alignment, counts, the plane
    d = {k: torch.from_numpy(np.ascontiguousarray(v, t)).cuda() for k, v, t in
         (("ids", good["ids"], np.int64), ("sf", good["sf"], np.int64), ("dirs", good["dirs"], np.int32),
          ("gains", good["gains"], np.float32), ("cf", good["cf"], np.int64), ("bf", good["bf"], np.int64))}
    dp = torch.from_numpy(pcm).cuda()
    o16 = torch.zeros(2 * 2048 + 8, dtype=torch.int16, device="cuda")
    o32 = torch.zeros(2 * 2048 + 8, dtype=torch.float32, device="cuda")

    def dev(off=None, n_chunks=2, n_total=4, plane=2048, n_mixes=2):
        p = {k: _vp(v) for k, v in dict(d, pcm=dp, o16=o16, o32=o32).items()}
        if off:
            p[off[0]] = C.c_void_p(p[off[0]].value + off[1])
        rc = L.jdsp_binaural_render_dev(h._h, p["pcm"], p["ids"], p["sf"], p["dirs"], p["gains"], p["cf"], p["bf"], n_mixes,
                                        n_chunks, n_total, p["o16"], p["o32"], plane)
        return rc, L.jdsp_last_error(eng._h).decode()

    eng._use_torch_stream()
    for off in (("pcm", 2), ("o16", 2), ("o32", 4), ("ids", 4), ("sf", 4), ("cf", 4), ("bf", 4), ("dirs", 2), ("gains", 2)):
        rc, text = dev(off=off)
        assert rc == EINVAL and "aligned" in text, (off, text)
    for kw, text in ((dict(n_chunks=5), "more chunks than live streams"), (dict(n_chunks=-1), "< 0"), (dict(n_total=-1), "< 0"),
                     (dict(plane=2047), "plane must be even"), (dict(plane=2046), "do not fit in plane")):
        rc, got = dev(**kw)
        assert rc == EINVAL and text in got, (kw, got)
    # nothing to do: launches nothing, changes nothing
    assert dev(n_mixes=0, n_chunks=0, n_total=0)[0] == 0 and dev(n_total=0)[0] == 0
    torch.cuda.synchronize()
    out = call(bf=[0, 0, 0])
    assert not as_np(out[0]).any()
    after = h.streams_state(every)
    for x, y in zip(before, after):
        assert same_bits(x, y)
    # and the handle still renders
    assert dev()[0] == 0
    torch.cuda.synchronize()
    assert h.streams_state([1])[3][0] == 1 and o16[:2048].any()
    h.close()
