"""BASELINE config 2's production kernel where its persistent loop actually loops.

fastconv1024_pairs_kernel (256-tap HRIR pair, 769-sample blocks) launches min(n_out_blocks, 3072) waves; each
walks e, e + grid, e + 2 grid ... with the next block's PCM requested one iteration ahead and stores whichever
sample pairing is dword-aligned at that block's odd-length output address.  The other fast-convolution tests stay
below 3,072 blocks, where every wave runs once.  Here: 7,531 blocks (> 2 x 3,072 and not a multiple of it), one
and two filters, against the CPU oracle (Fast_Convolution_Based_3DAudio_Impl.cpp:125-171 restated) -- pre-cast
1e-5 of the peak, int16 +-1 LSB -- as one call, as two calls whose cut is not a multiple of the grid, with a first
call that lies inside the silent head (fewer blocks than the history), and bit-identical to the same stream fed in
calls of at most 3,000 blocks (one loop iteration per wave).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5
NB = 7531
BLOCK = 769


@pytest.fixture(scope="module")
def eng():
    import jeicyboodsp_amd
    e = jeicyboodsp_amd.Engine(0)
    yield e
    e.close()


def _pcm(seed, n, sigma=2000.0):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.normal(0.0, sigma, n)), -32768, 32767).astype(np.int16)


def _hrir(seed, n_filters):
    rng = np.random.default_rng(seed)
    h = np.stack([rng.normal(size=256) * np.exp(-np.arange(256) / (40.0 + 15.0 * f)) for f in range(n_filters)])
    # unit energy: the output stays at the input's level (sigma 2000), inside int16; pre-cast values past +-32768 are
    # compared across the wrap in test_fastconv_streams_gpu.py::test_wrap_like_the_oracle_cast
    return h / np.sqrt((h * h).sum(axis=1, keepdims=True))


def _feed(fc, pcm, cuts):
    """process() over consecutive slices of `cuts` blocks; concatenated (int16 [F, n], pre-cast [F, n])."""
    outs, pres, pos = [], [], 0
    for n in cuts:
        o, p = fc.process(pcm[pos * BLOCK:(pos + n) * BLOCK], want_precast=True)
        outs.append(o); pres.append(p); pos += n
    assert pos * BLOCK == pcm.size
    return np.concatenate(outs, axis=1), np.concatenate(pres, axis=1)


@pytest.mark.parametrize("n_filters", [1, 2])
def test_persistent_loop_runs_three_times_and_matches_the_oracle(eng, oracle, n_filters):
    h = _hrir(10 + n_filters, n_filters)
    pcm = _pcm(20 + n_filters, NB * BLOCK)
    fc = eng.fastconv(h, 1024)
    assert fc.block == BLOCK and fc.hist_blocks == 1
    one, one_pre = _feed(fc, pcm, [NB])                                  # one call: three loop iterations per wave
    assert one.shape == (n_filters, (NB - 1) * BLOCK)
    for f in range(n_filters):
        o_out, o_pre = oracle.fastconv_stream(pcm, h[f], 1024)
        assert o_out.shape == one[f].shape
        assert np.abs(one_pre[f] - o_pre).max() < TOL * np.abs(o_pre).max()
        assert np.abs(one[f].astype(np.int32) - o_out.astype(np.int32)).max() <= 1
    # the cut at 3,333 is neither a multiple of the grid nor of anything else in the kernel; the second call
    # (4,198 blocks) loops twice with a partial last round and starts from the carried history
    fc.reset()
    two, two_pre = _feed(fc, pcm, [3333, NB - 3333])
    assert np.array_equal(two, one) and np.array_equal(two_pre.view(np.uint32), one_pre.view(np.uint32))
    # a first call inside the silent head (1 block < history + 1: nothing comes out), then the rest
    fc.reset()
    head, head_pre = _feed(fc, pcm, [1, 3332, NB - 3333])
    assert np.array_equal(head, one) and np.array_equal(head_pre.view(np.uint32), one_pre.view(np.uint32))
    # every wave loops once: calls of at most 3,000 blocks
    fc.reset()
    small, small_pre = _feed(fc, pcm, [3000, 3000, NB - 6000])
    assert np.array_equal(small, one) and np.array_equal(small_pre.view(np.uint32), one_pre.view(np.uint32))
    fc.close()


def test_exact_multiples_of_the_grid_and_one_more(eng, oracle):
    """Block counts that end a round exactly (3,072 and 6,144 output blocks) and one past it."""
    h = _hrir(31, 2)
    for n_out in (3072, 3073, 6144, 6145):
        nb = n_out + 1
        pcm = _pcm(n_out, nb * BLOCK)
        fc = eng.fastconv(h, 1024)
        out, pre = fc.process(pcm, want_precast=True)
        for f in range(2):
            o_out, o_pre = oracle.fastconv_stream(pcm, h[f], 1024)
            assert np.abs(pre[f] - o_pre).max() < TOL * np.abs(o_pre).max()
            assert np.abs(out[f].astype(np.int32) - o_out.astype(np.int32)).max() <= 1
        fc.close()
