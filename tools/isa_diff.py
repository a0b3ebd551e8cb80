#!/usr/bin/env python3
"""isa_diff.py emit DIR [TREE]   every csrc/*.hip of TREE (default: this one) -> DIR/<file>.s, common + per-file flags
isa_diff.py cmp OLD_DIR NEW_DIR  kernel by kernel (runs here, no GPU): kernels that left or came; of the rest how many
are text-identical (labels normalised); for every other one the launch resources (LDS, scratch, SGPRs, VGPRs in
allocation granules of 8) and the counts of floating-point, conversion and memory opcodes, which must be equal,
and the integer / scalar / wait opcodes whose counts differ."""
import collections, glob, os, re, subprocess, sys

FP_MEM = re.compile(r"v_pk_|v_\w*_(f16|f32|f64)|v_fma|v_cvt|v_exp|v_log|v_rcp|v_rsq|v_sqrt|v_div|v_mfma|"
                    r"ds_|global_|buffer_|flat_|scratch_|s_load")
RES = ("group_segment_fixed_size", "private_segment_fixed_size", "next_free_sgpr", "next_free_vgpr")


def emit(out, tree=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")):
    sys.path.insert(0, os.path.abspath(tree))
    import __graft_entry__ as g
    os.makedirs(out, exist_ok=True)
    for src in sorted(glob.glob(os.path.join(g.CSRC, "*.hip"))):
        base = os.path.basename(src)
        subprocess.check_call([g.HIPCC] + g.HIP_FLAGS + g.file_flags().get(base, []) +
                              ["--cuda-device-only", "-S", src, "-o", os.path.join(out, base[:-4] + ".s")])


def kernels(path):
    """{kernel: (normalised text, resources, opcode counts)}"""
    text = re.sub(r"\.LBB\d+_|\.Lfunc_(begin|end)\d+|\.Ltmp\d+", lambda m: re.sub(r"\d+_?$", "", m.group(0)), open(path).read())
    out = {}
    for name in re.findall(r"\.amdhsa_kernel (\w+)", text):
        start = text.index("\n%s:" % name)
        body = text[start:text.index(".end_amdhsa_kernel", start)]
        res = {k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1)) for k in RES}
        res["next_free_vgpr"] = -(-res["next_free_vgpr"] // 8) * 8
        ops = collections.Counter(re.findall(r"^\s+([a-z]\w+)", body.split("s_endpgm")[0], re.M))
        out[name] = (body, res, ops)
    return out


def cmp(old_dir, new_dir):
    bad = 0
    for old in sorted(glob.glob(os.path.join(old_dir, "*.s"))):
        a, b = kernels(old), kernels(os.path.join(new_dir, os.path.basename(old)))
        both = sorted(set(a) & set(b))
        same = [k for k in both if a[k][0] == b[k][0]]
        print("%s: %d kernels, %d text-identical" % (os.path.basename(old), len(both), len(same)))
        for k in sorted(set(a) - set(b)):
            print("  left   " + k)
        for k in sorted(set(b) - set(a)):
            print("  CAME   " + k); bad += 1
        for k in sorted(set(both) - set(same)):
            (_, ra, oa), (_, rb, ob) = a[k], b[k]
            diff = {o: (oa[o], ob[o]) for o in sorted(set(oa) | set(ob)) if oa[o] != ob[o]}
            must = {o: v for o, v in diff.items() if FP_MEM.match(o)}
            ok = ra == rb and not must
            bad += not ok
            print("  %s %s\n      resources %s%s\n      may differ: %s" % (
                "equal " if ok else "DIFFER", k, ra, "" if ra == rb else " -> %s" % rb,
                ", ".join("%s %d->%d" % (o, v[0], v[1]) for o, v in diff.items() if o not in must) or "-"))
            if must:
                print("      MUST NOT differ: %s" % must)
    print("FAIL: %d" % bad if bad else "OK")
    return bad


if __name__ == "__main__":
    sys.exit(emit(*sys.argv[2:]) if sys.argv[1] == "emit" else cmp(*sys.argv[2:]))
