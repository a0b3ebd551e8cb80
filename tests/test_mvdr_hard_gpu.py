"""GPU: the two-microphone MVDR on the scenes, delays and matrices white noise does not reach (tests/mvdr_cases.py),
through each of its three block paths:
  mvdr_pairs_kernel, weights from the table   _process in one call, in calls of 1, 3, 9 and 17 blocks, device pointers
  mvdr_pairs_kernel, weights computed         1,100 blocks with 1,099 estimation events in one call
  mvdr_kernel                                 jdsp_mvdr_apply under caller matrices, and the sharded run's finish
All against the C oracle at the header's bars, and held to max(4 x plain FP32's share, 0.1) of the 1e-5 bar
(mvdr_cases.check); tests/test_mvdr_hard_cpu.py shows that plain FP32 takes at most 0.05 of it here.
Run with -s for the share of the bar per case (profiles/r24_mvdr_hard.txt holds them)."""
import numpy as np
import pytest

import mvdr_cases as H

pytestmark = pytest.mark.gpu
CALLS = [1, 3, 9, 17]
FRACTIONAL = 1.37 * 6.25e-5

_oracle_cache = {}
_plain_cache = {}


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def oracle_case(orc, name, d_time, n_blocks=H.N_BLOCKS):
    """(o_out, o_pre, corr, trace) of one case, computed once, shared and read-only"""
    key = (name, d_time, n_blocks)
    if key not in _oracle_cache:
        res = orc.mvdr_stream(*H.cached_scene(name, n_blocks), d_time)
        for a in res:
            a.setflags(write=False)
        _oracle_cache[key] = res
    return _oracle_cache[key]


def plain_case(orc, name, d_time):
    """plain FP32's share of the bar on the 30-block case"""
    key = (name, d_time)
    if key not in _plain_cache:
        s, same = H.share(H.ref32(*H.cached_scene(name), d_time)["pre"], oracle_case(orc, name, d_time)[1])
        assert same
        _plain_cache[key] = s
    return _plain_cache[key]


def figures(title, name, shares):
    print("share of the bar %-22s %-20s %s" % (title, name, "  ".join("%g: %.4f (x%.1f)" % (d, s, s / p if p else 0.0)
                                                                        for d, (s, p) in shares.items())))


def assert_matrix(c, o_corr):
    scale = max(o_corr[0], o_corr[3], 1.0)
    assert abs(c[0] - o_corr[0]) <= 1e-12 * scale and abs(c[3] - o_corr[3]) <= 1e-12 * scale
    assert c[1] == 0.0 and c[2] == 0.0


@pytest.mark.parametrize("name", H.SCENES)
def test_one_call_holds_the_bar_at_every_delay(eng, oracle, name):
    """_process on host arrays, one call per delay: the tabled branch of mvdr_pairs_kernel; the matrix is the oracle's"""
    L, R = H.cached_scene(name)
    shares = {}
    for d_time in H.DELAYS:
        o_out, o_pre, o_corr, _ = oracle_case(oracle, name, d_time)
        p = plain_case(oracle, name, d_time)
        m = eng.mvdr(d_time)
        out, pre = m.process(L, R, want_precast=True)
        c = m.corr()
        m.close()
        shares[d_time] = (H.check(out, pre, o_out, o_pre, p), p)
        assert_matrix(c, o_corr)
        if name == "dead_right_in_pauses":               # singular: the non-finite value before the cast, 0 behind it
            assert not np.isfinite(pre).any() and not out.any()
    figures("one call", name, shares)


@pytest.mark.parametrize("name", H.SCENES)
def test_calls_of_any_length_give_the_same_bits(eng, oracle, name):
    """Calls of 1, 3, 9 and 17 blocks, cyclic, on one handle, then reset() and the one call again: the bytes of one call
    on a fresh handle (itself held to the oracle here)."""
    L, R = H.cached_scene(name)
    for d_time in (1e-4, -2.5e-3):
        o_out, o_pre, _, _ = oracle_case(oracle, name, d_time)
        m = eng.mvdr(d_time)
        want_out, want_pre = m.process(L, R, want_precast=True)
        H.check(want_out, want_pre, o_out, o_pre, plain_case(oracle, name, d_time))
        m.close()
        m = eng.mvdr(d_time)
        outs, pres, pos, k = [], [], 0, 0
        while pos < H.N_BLOCKS:
            n = min(CALLS[k % len(CALLS)], H.N_BLOCKS - pos)
            o, p = m.process(L[pos * 512:(pos + n) * 512], R[pos * 512:(pos + n) * 512], want_precast=True)
            outs.append(o)
            pres.append(p)
            pos += n
            k += 1
        assert np.concatenate(outs).tobytes() == want_out.tobytes(), d_time
        assert np.concatenate(pres).tobytes() == want_pre.tobytes(), d_time
        m.reset()
        out, pre = m.process(L, R, want_precast=True)
        m.close()
        assert out.tobytes() == want_out.tobytes() and pre.tobytes() == want_pre.tobytes(), d_time


@pytest.mark.parametrize("name", H.SCENES)
def test_device_pointer_entry_gives_the_host_entrys_bits(eng, oracle, name):
    import torch
    L, R = H.cached_scene(name)
    o_out, o_pre, _, _ = oracle_case(oracle, name, FRACTIONAL)
    m = eng.mvdr(FRACTIONAL)
    want_out, want_pre = m.process(L, R, want_precast=True)
    m.close()
    H.check(want_out, want_pre, o_out, o_pre, plain_case(oracle, name, FRACTIONAL))
    m = eng.mvdr(FRACTIONAL)
    out, pre = m.process(torch.from_numpy(L.copy()).cuda(), torch.from_numpy(R.copy()).cuda(), want_precast=True)
    torch.cuda.synchronize()
    out, pre = out.cpu().numpy(), pre.cpu().numpy()
    m.close()
    assert out.tobytes() == want_out.tobytes() and pre.tobytes() == want_pre.tobytes()


@pytest.mark.parametrize("name", H.NEVER_LOUD)
def test_untabled_branch_computes_its_weights_per_block(eng, oracle, name):
    """1,100 blocks on which the VAD's channel never speaks: 1,099 estimation events, at least 1,024 and at least a
    quarter of the blocks, so mvdr_pairs_kernel computes the weights of every block itself (mvdr_tabled() is false).
    Held to the plain-FP32 share of the 30-block case of the same scene and delay."""
    nb = 1100
    L, R = H.cached_scene(name, nb)
    shares = {}
    for d_time in (1e-4, FRACTIONAL, -2.5e-3):
        o_out, o_pre, o_corr, trace = oracle_case(oracle, name, d_time, nb)
        events = int(np.count_nonzero(np.diff(trace[:, 0], prepend=0.0) != 0))
        assert events >= 1024 and 4 * events >= nb
        p = plain_case(oracle, name, d_time)
        m = eng.mvdr(d_time)
        out, pre = m.process(L, R, want_precast=True)
        c = m.corr()
        m.close()
        shares[d_time] = (H.check(out, pre, o_out, o_pre, p), p)
        assert_matrix(c, o_corr)
        # the same stream in two calls of 550 blocks, under 1,024 events each: the weights come from the table, the bits stay
        m = eng.mvdr(d_time)
        halves = [m.process(L[k * 550 * 512:(k + 1) * 550 * 512], R[k * 550 * 512:(k + 1) * 550 * 512], want_precast=True)
                  for k in range(2)]
        m.close()
        assert np.concatenate([h[0] for h in halves]).tobytes() == out.tobytes(), d_time
        assert np.concatenate([h[1] for h in halves]).tobytes() == pre.tobytes(), d_time
    figures("untabled, 1100 blocks", name, shares)


@pytest.mark.parametrize("matrix", list(H.MATRICES))
def test_apply_under_caller_matrices(eng, oracle, matrix):
    """jdsp_mvdr_apply (mvdr_kernel) on the loud blocks 9..17 of `white` with matrices no stream arrives at"""
    L, R = H.loud_blocks(*H.cached_scene("white"))
    corr = np.array(H.MATRICES[matrix])
    shares = {}
    for d_time in H.APPLY_DELAYS:
        o_out, o_pre = oracle.mvdr_apply(L, R, corr, d_time)
        p, same = H.share(H.apply_ref32(L, R, corr, d_time)["pre"], o_pre)
        assert same
        m = eng.mvdr(d_time)
        out, pre = m.apply(L, R, corr, want_precast=True)
        m.close()
        shares[d_time] = (H.check(out, pre, o_out, o_pre, p), p)
    figures("apply", matrix, shares)


@pytest.mark.parametrize("name", H.SCENES)
def test_apply_and_estimate_with_the_streams_own_matrix(eng, oracle, name):
    """estimate_corr on the scene's pause frames reproduces the matrix the stream ends with (diagonal to 1e-12,
    off-diagonal exactly 0), and jdsp_mvdr_apply with that matrix over the scene's blocks 9..17 holds the bar."""
    L, R = H.cached_scene(name)
    Ll, Rl = H.loud_blocks(L, R)
    shares = {}
    for d_time in (1e-4, FRACTIONAL):
        _, _, o_corr, _ = oracle_case(oracle, name, d_time)
        o_out, o_pre = oracle.mvdr_apply(Ll, Rl, o_corr, d_time)
        p, same = H.share(H.apply_ref32(Ll, Rl, o_corr, d_time)["pre"], o_pre)
        assert same
        m = eng.mvdr(d_time)
        out, pre = m.apply(Ll, Rl, o_corr, want_precast=True)
        shares[d_time] = (H.check(out, pre, o_out, o_pre, p), p)
        flags = H.ref64(L, R, d_time)["flags"]
        got = m.estimate_corr(H.pause_frames(L, flags), H.pause_frames(R, flags), np.zeros(4))
        m.close()
        assert_matrix(got, o_corr)
    figures("apply, own matrix", name, shares)


@pytest.mark.parametrize("name", ["lowpassed", "gain_mismatch", "quiet_left", "full_scale"])
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_run_holds_the_bar_before_the_cast(eng, oracle, world, name):
    """Simulated ranks on one GPU (all-gathers = concatenations), mvdr_kernel with a rank's version offsets, and
    jdsp_mvdr_shard_finish_dev's precast output, which no test had asked for."""
    import torch
    from jeicyboodsp_amd import sharding
    L, R = H.cached_scene(name)
    tl, tr = torch.from_numpy(L.copy()).cuda(), torch.from_numpy(R.copy()).cuda()
    shares = {}
    for d_time in (1e-4, -2.5e-3):
        o_out, o_pre, _, _ = oracle_case(oracle, name, d_time)
        ranks = []
        for r in range(world):
            b0, cnt = sharding.split_even(H.N_BLOCKS, r, world)
            ext0 = max(b0 - 1, 0)
            ranks.append(dict(m=eng.mvdr(d_time), ext0=ext0, b0=b0, b1=b0 + cnt,
                              l=tl[ext0 * 512:(b0 + cnt) * 512].clone(), r=tr[ext0 * 512:(b0 + cnt) * 512].clone()))
        flags = torch.cat([k["m"].shard_vad(k["l"], k["r"], k["ext0"], k["b0"], k["b1"], H.N_BLOCKS) for k in ranks]).contiguous()
        sums = torch.stack([k["m"].shard_summary(flags) for k in ranks]).contiguous()
        res = [k["m"].shard_finish(sums, world, r, want_precast=True) for r, k in enumerate(ranks)]
        torch.cuda.synchronize()
        out = torch.cat([o for o, _ in res]).cpu().numpy()
        pre = torch.cat([p for _, p in res]).cpu().numpy()
        for k in ranks:
            k["m"].close()
        p = plain_case(oracle, name, d_time)
        shares[d_time] = (H.check(out, pre, o_out, o_pre, p), p)
    figures("sharded, world %d" % world, name, shares)


def test_vad_threshold_blocks_and_the_stream_built_on_them(eng, oracle):
    """Energy sums of 716,799, 716,800 and 716,801 (700 x 1024 and its neighbours) decide quiet, quiet, voice, and the
    sums come back exact.  Then a stream whose first pause is the 716,800 block nine times over and whose second holds
    the 716,801 block (voice: it resets the run counter) against the oracle."""
    v, e, _ = eng.vad_blocks(H.vad_edge_blocks(), "mvdr")
    assert list(v) == [0, 0, 1] and tuple(int(x) for x in e) == H.VAD_SUMS
    L, R, flags = H.vad_edge_stream()
    shares = {}
    for d_time in (1e-4, -2.5e-3):
        o_out, o_pre, o_corr, trace = oracle.mvdr_stream(L, R, d_time)
        assert list(np.flatnonzero(np.diff(trace[:, 0], prepend=0.0) != 0)) == list(range(1, 9)) + [19, 22]
        p, same = H.share(H.ref32(L, R, d_time)["pre"], o_pre)
        assert same
        m = eng.mvdr(d_time)
        out, pre = m.process(L, R, want_precast=True)
        c = m.corr()
        m.close()
        shares[d_time] = (H.check(out, pre, o_out, o_pre, p), p)
        assert_matrix(c, o_corr)
    figures("one call", "vad_edge_stream", shares)
