"""Writes tests/golden/streamfilter.npz: what the reference's own 7Band_GEQ.cpp and NormalLMS.cpp write for seeded
int16 streams, and the 42 coefficients the former computes.  Runs where a checkout of the reference is at hand
(authoring only):

    python tests/golden/make_golden_streamfilter.py <reference dir>

Each program is compiled as it lies (g++ -O2 -w -fpermissive) from a driver translation unit written to a temporary
directory, which renames the reference's main() and includes the reference source by path.  Both include fftw3.h and
use nothing from it: an empty file of that name in the temporary directory stands in.  One process per stream, so
every stream starts from the zero state.  Only the streams, the output files' samples and the coefficients are stored."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import streamfilter_ref as R  # noqa: E402

DRIVER = """#include <stdlib.h>
#include <stdio.h>
#define main ref_main
#include "%s"
#undef main
int main(int argc, char **argv) {
    ref_main(argc, argv);
%s
    return 0;
}
"""
DUMP_COEFF = """    FILE *fc = fopen("coeff.bin", "wb");
    fwrite(rgdBandCoeff, sizeof(double), 42, fc);
    fclose(fc);"""


def build(ref_dir, tmp, source, exe, tail=""):
    open(os.path.join(tmp, "fftw3.h"), "w").close()
    src = os.path.join(tmp, exe + ".cpp")
    with open(src, "w") as f:
        f.write(DRIVER % (os.path.join(ref_dir, source), tail))
    subprocess.check_call(["g++", "-O2", "-w", "-fpermissive", "-I" + tmp, src, "-o", os.path.join(tmp, exe)])
    return os.path.join(tmp, exe)


def write_wav(path, pcm):
    with open(path, "wb") as f:
        f.write(struct.pack("<44x"))
        f.write(np.asarray(pcm, "<i2").tobytes())


def run(exe, tmp, args):
    subprocess.run([exe] + args, cwd=tmp, stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL, check=True)


def main():
    ref_dir = os.path.abspath(sys.argv[1])
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        geq = build(ref_dir, tmp, "7Band_GEQ.cpp", "geq", DUMP_COEFF)
        nlms = build(ref_dir, tmp, "NormalLMS.cpp", "nlms")
        p = lambda name: os.path.join(tmp, name)  # noqa: E731
        for name, pcm in R.geq_families().items():
            write_wav(p("in.wav"), pcm)
            run(geq, tmp, [p("in.wav"), p("out.raw")])
            out["geq_pcm_" + name] = pcm
            out["geq_out_" + name] = np.fromfile(p("out.raw"), "<i2")
            assert len(out["geq_out_" + name]) == len(pcm)
        out["geq_coeff"] = np.fromfile(p("coeff.bin"), "<f8").reshape(7, 2, 3)
        for name, (x, ref) in R.nlms_families().items():
            write_wav(p("in.wav"), x)
            np.asarray(ref, "<i2").tofile(p("ref.raw"))
            run(nlms, tmp, [p("in.wav"), p("ref.raw"), p("est.raw"), p("err.raw")])
            out["nlms_in_" + name], out["nlms_ref_" + name] = x, ref
            out["nlms_est_" + name] = np.fromfile(p("est.raw"), "<i2")      # from the second block on
            out["nlms_err_" + name] = np.fromfile(p("err.raw"), "<i2")
            assert len(out["nlms_est_" + name]) == len(x) - R.NLMS_BLOCK
    path = os.path.join(HERE, "streamfilter.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
