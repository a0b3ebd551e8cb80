"""CPU tests of batched reverberation's boundary: libjdsp.so exports the eight jdsp_reverb_* entries and the Python
binding knows them, the header states the contract (limits, layout, the appended-zeros note on the tail, the arithmetic),
the ABI version stays 2, and the "Graph capture" conventions name the device entry in class S.  No compute here."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jdsp.h")
LIB = os.path.join(ROOT, "jeicyboodsp_amd", "libjdsp.so")
ENTRIES = ("jdsp_reverb_create", "jdsp_reverb_destroy", "jdsp_reverb_n_irs", "jdsp_reverb_n_part", "jdsp_reverb_block_len",
           "jdsp_reverb_batch_reserve", "jdsp_reverb_batch_dev", "jdsp_reverb_batch")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build_hip()
    return C.CDLL(LIB)


def test_the_library_exports_the_eight_entries_and_the_binding_knows_them(lib):
    missing = [n for n in ENTRIES if not hasattr(lib, n)]
    assert not missing, missing
    import jeicyboodsp_amd
    from jeicyboodsp_amd.engine import L, Engine, Reverb
    for n in ENTRIES:
        assert getattr(L, n).argtypes is not None, n
    assert len(L.jdsp_reverb_batch_dev.argtypes) == 10 and len(L.jdsp_reverb_batch.argtypes) == 10
    assert callable(Engine.reverb) and callable(Reverb.process_batch) and callable(Reverb.reserve_batch)
    # handles of nothing: the getters answer 0, destroy takes NULL, the batch entries refuse it
    for n in ("jdsp_reverb_n_irs", "jdsp_reverb_n_part", "jdsp_reverb_block_len", "jdsp_reverb_destroy"):
        assert getattr(L, n)(None) == 0, n
    assert L.jdsp_reverb_batch_reserve(None, 1, 1) == jeicyboodsp_amd._lib.EINVAL
    assert L.jdsp_reverb_batch_dev(None, None, None, None, None, None, 0, 0, None, None) == jeicyboodsp_amd._lib.EINVAL
    assert L.jdsp_reverb_create(None, None, 1, 1, None) == jeicyboodsp_amd._lib.EINVAL


def test_the_header_states_the_contract(lib):
    txt = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, code), n
    assert re.search(r"#define\s+JDSP_ABI_VERSION\s+2\b", txt)
    lib.jdsp_abi_version.restype = C.c_int
    assert lib.jdsp_abi_version() == 2
    flat = re.sub(r"[\s*]+", " ", txt)
    sec = flat[flat.index("batched reverberation: ragged utterances"):flat.index("typedef struct jdsp_reverb jdsp_reverb;")]
    for phrase in ("1 <= n_taps <= 7680", "1 <= n_irs <= 16384", "jdsp_denoise_batch_dev's", "appends P blocks of zeros",
                   "512 zeros in front of it", "truncate toward zero", "gain[u] 2^-10", "p ascending", "clamped into [0, n_irs)",
                   "class S", "4,160 bytes per reserved block", "ZERO outside the spans", "62,400"):
        assert phrase in sec, phrase
    # the conventions: the entry is stateless under graph capture, and its workspace has a reserve call
    conv = flat[flat.index("GRAPH CAPTURE."):flat.index("Class D, state on the device only")]
    assert "jdsp_reverb_batch_dev" in conv[conv.index("Class S, stateless"):]
    assert "jdsp_reverb_batch_reserve" in flat[:flat.index("GRAPH CAPTURE.")]
