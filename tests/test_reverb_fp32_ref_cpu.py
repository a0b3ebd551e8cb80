"""What plain FP32 makes of the reverberator's batches (CPU): reverb_cases.restate32 -- numpy's float32 rfft, complex64
spectra, never upcast, the bank spectra rounded from FP64 -- on every utterance of every bank's batch, against the FP64
direct convolution (reverb_ref) and both bars.

These are conditions on the CHOICE OF CASES, not measurements of the library: the bars are not vacuous (FP32 can meet
them on every case the device test runs), and a case that fails here is wrong for this algorithm -- it is to be
changed, not the bar.  Also asserted: the batches hold what they claim (every length, family and gain, shared responses,
a wrap that wraps, utterances whose bars are zero).

The table this prints (pytest -s) is recorded in profiles/r29_reverb_batch.txt.
"""
import numpy as np
import pytest

import reverb_cases as K
import reverb_ref


@pytest.fixture(scope="module")
def table():
    """bank -> (worst fraction of the global bar, of the local bar, int16 samples more than one step off)"""
    rows = {}
    for name in K.banks():
        b = K.batch(name)
        worst = [0.0, 0.0, 0]
        for u in b.utts:
            y = K.restate32(u.x, b.taps[u.ir], u.gain)
            g, loc = K.ratios_of(y, u)
            own, far = K.int16_rules(K.cast_i16(y), y, u)
            worst = [max(worst[0], g), max(worst[1], loc), worst[2] + far]
        rows[name] = tuple(worst)
    print("\nplain FP32 partitioned sum, worst fraction of each bar per bank (global, local, int16 > 1 step off)")
    for name, (g, loc, far) in rows.items():
        print("  %-10s P = %2d %8.4f %8.4f %6d" % (name, K.n_part(K.banks()[name].shape[1]), g, loc, far))
    return rows


@pytest.mark.parametrize("name", list(K.banks()))
def test_plain_fp32_meets_both_bars(table, name):
    g, loc, far = table[name]
    assert g <= 1.0 and loc <= 1.0 and far == 0, (name, g, loc, far)


def test_the_batches_hold_what_they_claim():
    assert [K.n_part(h.shape[1]) for h in K.banks().values()] == [1, 1, 2, 3, 15, 15, 3, 1]
    assert K.banks()["tap1"][0].tolist() == [0.75] and abs(K.banks()["highpass"][0].sum()) < 1e-12
    assert np.count_nonzero(K.banks()["rir7169"][0]) < 7169 and K.banks()["rir7169"].shape == (3, 7169)
    for name, taps in K.banks().items():
        b, P = K.batch(name), K.n_part(taps.shape[1])
        lens = {u.x.size // K.B for u in b.utts}
        assert lens >= {0, 1, 2, max(P - 1, 0), P, P + 1, K.G - 1, K.G, K.G + 1, 2 * K.G + 1}, (name, lens)
        assert {u.family for u in b.utts if u.x.size >= 3 * K.B} == set(K.FAMILIES), name
        assert {u.gain for u in b.utts if u.x.size} == set(K.GAINS), name
        irs = [u.ir for u in b.utts]
        assert {0, taps.shape[0] - 1} <= set(irs) and max(irs.count(i) for i in set(irs)) >= 3, name
        # exact zeros are asked of silence, of gain 0 on a loud utterance, and nowhere else
        zero = [u for u in b.utts if K.must_be_zero(u)]
        assert any(u.gain == 0.0 and u.x.any() for u in zero) and any(u.gain != 0.0 and not u.x.any() for u in zero), name
        assert all(u.gain == 0.0 or not u.x.any() for u in zero), name
        for u in b.utts:
            assert u.w.shape == u.x.shape == u.local_bar.shape


def test_the_reference_is_the_definition():
    """np.convolve against the double loop of the definition, on a short utterance"""
    rng = np.random.default_rng(5)
    x = rng.integers(-32768, 32768, 40).astype(np.int16)
    h = rng.normal(size=7)
    want = [-3.0 * sum(h[k] * float(x[t - k]) for k in range(7) if t - k >= 0) for t in range(40)]
    assert np.allclose(reverb_ref.reverb(x, h, -3.0), want, rtol=1e-13, atol=1e-9)


def test_the_restatement_in_fp64_is_the_reference():
    """the partitioned sum itself, in FP64, equals the direct convolution to FP64 round-off: partitions, lead zeros and
    kept halves are right"""
    for name in ("taps513", "rir7169"):
        b = K.batch(name)
        u = max(b.utts, key=lambda u: u.x.size if u.x.any() and u.gain else 0)
        h = b.taps[u.ir]
        P, nb = K.n_part(h.size), u.x.size // K.B
        hp = np.zeros(P * K.B)
        hp[:h.size] = h
        H = np.fft.rfft(np.concatenate([hp.reshape(P, K.B), np.zeros((P, K.B))], axis=1), axis=1)
        xz = np.concatenate([np.zeros(K.B), u.x.astype(np.float64)])
        X = np.fft.rfft(np.stack([xz[c * K.B:c * K.B + 2 * K.B] for c in range(nb)]), axis=1)
        Y = np.zeros_like(X)
        for p in range(min(P, nb)):
            Y[p:] += X[:nb - p] * H[p]
        y = u.gain * np.fft.irfft(Y, n=2 * K.B, axis=1)[:, K.B:].reshape(-1)
        assert np.abs(y - u.w).max() < 1e-9 * np.abs(u.w).max(), name


def test_the_wrap_bank_wraps():
    for name in K.WRAP_BANKS:
        w = np.concatenate([u.w for u in K.batch(name).utts])
        assert np.count_nonzero(np.abs(w) > 32768.0) >= 1000 and np.count_nonzero(np.abs(w) > 98304.0) > 0, name


def test_the_local_bar_is_tighter_where_the_utterance_is_quiet():
    for name in ("taps512", "taps1025"):
        for u in K.batch(name).utts:
            if u.family == "loud_then_quiet" and u.x.size >= 3 * K.B and u.gain:
                assert u.global_bar / u.local_bar.min() >= 30.0, (name, u.global_bar / u.local_bar.min())
