"""Writes tests/golden/timedomain.npz: what the reference's own PitchEstimation_method2.cpp and _method3.cpp print
for seeded int16 streams.  Runs where a checkout of the reference is at hand (authoring only):

    python tests/golden/make_golden_timedomain.py <reference dir>

Each program is compiled as it lies (g++ -O2 -w -fpermissive) from a driver translation unit written to a temporary
directory, which renames the reference's main() and includes the reference source by path; one process per stream, so
every stream starts from the zero keep buffer.  Only the streams and the printed numbers are stored."""
import os
import re
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import timedomain_ref as R  # noqa: E402

DRIVER = """#include <stdlib.h>
#define main ref_main
#include "%s"
#undef main
int main(int argc, char **argv) { ref_main(argc, argv); return 0; }
"""
LINE = re.compile(r"Estimation arg (-?\d+) , dMin (\S+) pitch")


def build(ref_dir, tmp, method):
    src = os.path.join(tmp, "drv%d.cpp" % method)
    exe = os.path.join(tmp, "pitch%d" % method)
    with open(src, "w") as f:
        f.write(DRIVER % os.path.join(ref_dir, "PitchEstimation_method%d.cpp" % method))
    subprocess.check_call(["g++", "-O2", "-w", "-fpermissive", src, "-o", exe])
    return exe


def run(exe, tmp, pcm):
    wav = os.path.join(tmp, "in.wav")
    with open(wav, "wb") as f:
        f.write(struct.pack("<44x"))
        f.write(np.asarray(pcm, "<i2").tobytes())
    out = subprocess.run([exe, wav], stdin=subprocess.DEVNULL, capture_output=True, check=True).stdout
    rows = LINE.findall(out.decode("latin-1"))
    assert len(rows) == len(pcm) // 512, (len(rows), len(pcm) // 512)
    return np.array([int(a) for a, _ in rows], np.int32), np.array([float(v) for _, v in rows], np.float64)


def streams():
    s = {
        "mixed": R.mixed(14, 40),
        "voiced": R.voiced(11, 16),
        "white": R.white(12, 12),
        "silence": R.silence(3),
        "constant": R.constant(3),
        "full_scale": R.full_scale(13, 8),
        # the keep buffer's hand-over at the head of a stream: one loud block after the initial zeros, then quiet
        "zero_keep": np.concatenate([R.white(15, 1, sigma=9000.0), R.voiced(16, 3, noise=30.0)]),
    }
    return s


def main():
    ref_dir = os.path.abspath(sys.argv[1])
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exes = {m: build(ref_dir, tmp, m) for m in (2, 3)}
        for name, pcm in streams().items():
            out["pcm_" + name] = pcm
            for m, exe in exes.items():
                out["arg%d_%s" % (m, name)], out["val%d_%s" % (m, name)] = run(exe, tmp, pcm)
    path = os.path.join(HERE, "timedomain.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
