"""Per-kernel comparison of two gfx950 assembly files (hipcc --cuda-device-only -S with the flags of generative-detection_amd/build.py)
of two versions of one source.  Kernels are matched by demangled name without the parameter list.  Per kernel: the resources the
compiler reports (VGPRs, AGPRs, scratch, LDS, occupancy) where they differ, then "same stream" when the instructions (comments and
labels stripped) are identical, or else the counts of the instruction classes a refactor must keep (v_mfma*, ds reads, ds writes,
buffer_load*, buffer_store*, s_barrier) and the histogram of every mnemonic whose count differs.
usage: python tools/isa_diff.py <parent.s> <new.s>"""
import collections
import re
import subprocess
import sys

RESOURCES = ["NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy"]
CLASSES = [("v_mfma", r"v_mfma"), ("ds read", r"ds_(read|load)"), ("ds write", r"ds_(write|store)"), ("buffer_load", r"buffer_load"),
           ("buffer_store", r"buffer_store"), ("s_barrier", r"s_barrier")]


def kernels(path):
    """{demangled name: (instruction list, {resource: value})} of every function of the file"""
    lines = open(path).read().splitlines()
    found, name, body = [], None, None
    for i, line in enumerate(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, body = m.group(1), []
        elif name and re.match(r"\.Lfunc_end\d+:", line):
            res = {}
            for after in lines[i:i + 60]:
                r = re.match(r";\s*(\w+):\s*(\d+)", after)
                if r and r.group(1) in RESOURCES:
                    res[r.group(1)] = int(r.group(2))
            found.append((name, body, res))
            name = None
        elif name:
            code = line.split(";")[0].strip()
            if code and not code.endswith(":") and not code.startswith("."):
                body.append(re.sub(r"\s+", " ", code))
    plain = subprocess.run(["c++filt"], input="\n".join(f[0] for f in found), capture_output=True, text=True).stdout.splitlines()
    return {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: (b, r) for d, (_, b, r) in zip(plain, found)}


def histogram(body):
    return collections.Counter(ins.split(" ")[0] for ins in body)


def main(parent_s, new_s):
    old, new = kernels(parent_s), kernels(new_s)
    worst = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("%s: only in the %s file" % (name, "new" if name in new else "parent"))
            worst = 1
            continue
        (ob, ores), (nb, nres) = old[name], new[name]
        moved = ["%s %s -> %s" % (k, ores.get(k), nres.get(k)) for k in RESOURCES if ores.get(k) != nres.get(k)]
        head = "%s: %s" % (name, "resources same" if not moved else "RESOURCES DIFFER " + ", ".join(moved))
        worst |= bool(moved)
        if ob == nb:
            print(head + "; same stream (%d instructions)" % len(nb))
            continue
        oh, nh = histogram(ob), histogram(nb)
        cls = []
        for label, pat in CLASSES:
            a = sum(c for m, c in oh.items() if re.match(pat, m))
            b = sum(c for m, c in nh.items() if re.match(pat, m))
            cls.append("%s %d%s" % (label, a, "" if a == b else " -> %d (DIFFERS)" % b))
            worst |= a != b
        print(head + "; instructions %d -> %d" % (len(ob), len(nb)))
        print("    classes: " + ", ".join(cls))
        diff = ["%s %d -> %d" % (m, oh[m], nh[m]) for m in sorted(set(oh) | set(nh)) if oh[m] != nh[m]]
        print("    mnemonics whose count differs: " + (", ".join(diff) if diff else "none (same histogram, other order or registers)"))
    return worst


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
