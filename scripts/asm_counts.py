#!/usr/bin/env python3
"""Register, code and wait-counter figures of kernels, read from the compiler's gfx950 assembly.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -S --cuda-device-only prad_api.hip -o prad_api.s
    python scripts/asm_counts.py prad_api.s sweep_fw_kernelILb1ELi8ELb0ELb1E [more name fragments ...]

For every kernel whose mangled name holds one of the fragments: VGPRs, SGPRs, spills, scratch, occupancy, code bytes,
the flat operations (all / inside a loop = between a label and a later branch back to it), and for every GROUP LOOP
(an innermost loop with at least 48 ds_add_u32: the plain groups of the walks) its waits: lgkmcnt(0) waits, and the
vmcnt waits in program order.

    python scripts/asm_counts.py --compare parent.s new.s

Are the kernels of two builds the same instruction text?  Per kernel the body between its entry label and .Lfunc_end, comments
stripped and the local labels (.LBB<n>_<m>, .Ltmp<n>, .Lfunc_end<n>) renumbered in order of appearance; prints one row per
kernel name of either side (lines of assembly, verdict) and exits 1 unless both sides hold the same names with identical bodies.
"""
import re
import sys


def kernels(path):
    name, body, out = None, [], {}
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            body.append(line.rstrip("\n"))
            if line.startswith(".Lfunc_end"):
                out[name] = {"body": body, "meta": {}}
                name = None
    # occupancy and code size from the comment block behind the body, the rest from the metadata records
    cur = None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
        m = re.match(r"^; (Occupancy|codeLenInByte)\s*[:=]\s*(\d+)", line)
        if m and cur in out:
            out[cur]["meta"].setdefault({"Occupancy": "occupancy", "codeLenInByte": "code_bytes"}[m.group(1)], int(m.group(2)))
        m = re.match(r"^\s+\.name:\s+(\S+)", line)
        if m:
            cur = m.group(1)
        m = re.match(r"^\s+\.(sgpr_count|sgpr_spill_count|vgpr_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", line)
        if m and cur in out:
            key = {"private_segment_fixed_size": "scratch_bytes"}.get(m.group(1), m.group(1))
            out[cur]["meta"][key] = int(m.group(2))
    return out


def loops(body):
    """(start, end) line ranges of loops: a label and the last branch back to it"""
    label_at = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            label_at[m.group(1)] = i
    spans = {}
    for i, l in enumerate(body):
        m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in label_at and label_at[m.group(1)] < i:
            s = label_at[m.group(1)]
            spans[s] = max(spans.get(s, 0), i)
    return sorted(spans.items())


def is_flat(l):
    return re.match(r"^\s+flat_(load|store|atomic)", l) is not None


def report(name, k):
    body, meta = k["body"], k["meta"]
    print("== %s" % name[:110])
    print("   " + "  ".join("%s=%s" % kv for kv in sorted(meta.items())))
    sp = loops(body)
    inloop = set()
    for s, e in sp:
        inloop.update(range(s, e + 1))
    flat = [i for i, l in enumerate(body) if is_flat(l)]
    print("   flat operations: %d, inside a loop: %d; global: %d; ds_add_u32: %d" % (
        len(flat), sum(i in inloop for i in flat), sum(bool(re.match(r"^\s+global_(load|store|atomic)", l)) for l in body),
        sum("ds_add_u32" in l for l in body)))
    for i in flat:
        print("      flat @%d %s   %s" % (i, "LOOP" if i in inloop else "    ", body[i].strip()))
    print("   s_load in a loop: %d" % sum(i in inloop and re.match(r"^\s+s_load_", body[i]) is not None for i in range(len(body))))
    inner = [(s, e) for s, e in sp if not any((s2 > s or e2 < e) and s2 >= s and e2 <= e for s2, e2 in sp)]
    n = 0
    for s, e in inner:
        seg = body[s:e + 1]
        adds = sum("ds_add_u32" in l for l in seg)
        if adds < 48:
            continue
        n += 1
        waits = [l.strip() for l in seg if "s_waitcnt" in l]
        lg0 = sum("lgkmcnt(0)" in w for w in waits)
        vm = [re.search(r"vmcnt\((\d+)\)", w).group(1) for w in waits if "vmcnt" in w]
        print("   group loop %d: lines %d-%d, ds_add %d, flat %d, global %d, s_load %d, lgkmcnt(0) waits %d, v_readlane %d, vmcnt waits: %s" % (
            n, s, e, adds, sum(is_flat(l) for l in seg), sum(bool(re.match(r"^\s+global_", l)) for l in seg),
            sum(bool(re.match(r"^\s+s_load_", l)) for l in seg), lg0, sum("v_readlane" in l for l in seg), " ".join(vm)))


def canonical(body):
    names, out = {}, []
    for l in body:
        l = l.split(";")[0].rstrip()
        if l:
            out.append(re.sub(r"\.L(?:BB\d+_\d+|tmp\d+|func_end\d+)", lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), l))
    return out


def compare(path_a, path_b):
    a, b = kernels(path_a), kernels(path_b)
    bad = 0
    print("| kernel | lines | verdict |\n|---|---|---|")
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            verdict = "MISSING in the %s build" % ("first" if name not in a else "second")
        else:
            verdict = "identical" if canonical(a[name]["body"]) == canonical(b[name]["body"]) else "DIFFERENT"
        bad += verdict != "identical"
        print("| `%s` | %d | %s |" % (name, len(canonical((a.get(name) or b[name])["body"])), verdict))
    print("\n%d kernels in the first build, %d in the second, %d not identical" % (len(a), len(b), bad))
    return 1 if bad else 0


def main():
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    ks = kernels(sys.argv[1])
    for name in sorted(ks):
        if any(f in name for f in sys.argv[2:]):
            report(name, ks[name])


if __name__ == "__main__":
    main()
