#!/usr/bin/env python3
"""Static census of kernels in a saved gfx950 device assembly (.s of -save-temps): instructions by kind, registers, scratch.
usage: isa_census.py kernels-hip-amdgcn-amd-amdhsa-gfx950.s [name-substring ...]   (default substring: k_flow_system)
The counts are static (every instruction of the kernel's text once), not what a thread executes."""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except Exception:
        return {n: n for n in names}


def kernels(path):
    """{symbol: {"body": [instructions], "text": [the raw lines, labels included], "vgpr", "sgpr", "scratch", "lds", "spills"}}"""
    text = open(path).read().split("\n")
    out, cur = {}, None
    for ln in text:
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", ln)
        if m:
            cur = m.group(1)
            out[cur] = {"body": [], "text": []}
            continue
        if cur is None:
            continue
        s = ln.strip()
        if s.startswith(".Lfunc_end") or s.startswith(".section") or s.startswith(".amdhsa_kernel"):
            cur = None
            continue
        out[cur]["text"].append(ln)
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        out[cur]["body"].append(s.split(";")[0].strip())
    # the metadata: one entry per kernel, opened by "  - .agpr_count:", fields at four spaces
    fields = {".vgpr_count": "vgpr", ".sgpr_count": "sgpr", ".private_segment_fixed_size": "scratch",
              ".group_segment_fixed_size": "lds", ".vgpr_spill_count": "spills"}
    entry = {}

    def close():
        if entry.get("name") in out:
            out[entry["name"]].update({k: v for k, v in entry.items() if k != "name"})
        entry.clear()

    for ln in text:
        if re.match(r"^  - \.\w+:", ln):
            close()
        m = re.match(r"^  [ -] (\.\w+):\s+(\S+)", ln)
        if m and m.group(1) == ".name":
            entry["name"] = m.group(2)
        elif m and m.group(1) in fields:
            entry[fields[m.group(1)]] = int(m.group(2))
    close()
    return out


def census(body):
    c = dict(total=len(body), vector=0, fp64=0, lds=0, vmem=0, vmem_x4=0, vmem_x2=0, salu=0, waitcnt=0, barrier=0)
    for ins in body:
        op = ins.split()[0]
        if op.startswith("v_"):
            c["vector"] += 1
            if re.search(r"_f64($|_)", op) or op.endswith("f64"):
                c["fp64"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            c["vmem"] += 1
            if op.endswith("dwordx4"):
                c["vmem_x4"] += 1
            elif op.endswith("dwordx2"):
                c["vmem_x2"] += 1
        elif op == "s_waitcnt":
            c["waitcnt"] += 1
        elif op == "s_barrier":
            c["barrier"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
    return c


def main():
    path, pats = sys.argv[1], sys.argv[2:] or ["k_flow_system"]
    ks = kernels(path)
    names = [n for n in ks if any(p in n for p in pats)]
    dm = demangle(names)
    for n in sorted(names, key=lambda n: dm[n]):
        k, c = ks[n], census(ks[n]["body"])
        short = dm[n].replace("papof::(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        print("%-40s VGPRs %3s  scratch %s B  LDS %s B | instructions %4d: vector %4d (fp64 %3d)  LDS %3d  vector-memory %3d "
              "(16-byte %2d, 8-byte %2d)  scalar %3d  s_waitcnt %3d  s_barrier %d" %
              (short, k.get("vgpr", "?"), k.get("scratch", "?"), k.get("lds", "?"), c["total"], c["vector"], c["fp64"],
               c["lds"], c["vmem"], c["vmem_x4"], c["vmem_x2"], c["salu"], c["waitcnt"], c["barrier"]))


if __name__ == "__main__":
    main()
