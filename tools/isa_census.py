#!/usr/bin/env python3
"""Static census of kernels in a saved gfx950 device assembly (.s of -save-temps): instructions by kind, registers, scratch.
usage: isa_census.py kernels-hip-amdgcn-amd-amdhsa-gfx950.s [name-substring ...]   (default substring: k_flow_system)
       isa_census.py --loops sor-hip-amdgcn-amd-amdhsa-gfx950.s [name-substring ...]    (default substring: k_sor_)
           the sweep loops of the solver kernels (label .. backward branch, at least 4 vector-memory stores): instructions by
           class, scalar ones included, and the s_waitcnt vmcnt(N) values in program order (profiles/slot_carry_isa.txt)
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


def loops(text, min_stores=4):
    """The loops of a kernel's text (label .. backward branch to it) that hold at least min_stores vector-memory stores -- the
    sweep loops of the solver kernels -- as lists of instructions, in program order of their closing branch."""
    labels, body, out = {}, [], []
    for ln in text:
        s = ln.split(";")[0].strip()
        if not s or s.startswith((".", "//")) and not s.endswith(":"):
            continue
        if s.endswith(":"):
            labels[s[:-1]] = len(body)
            continue
        body.append(s)
        m = re.match(r"s_c?branch\w*\s+(\S+)", s)
        if m and m.group(1) in labels:
            rng = body[labels[m.group(1)]:]
            if sum(1 for i in rng if re.match(r"(buffer|global|flat)_store", i)) >= min_stores:
                out.append(rng)
    return out


def loop_census(rng):
    op = [i.split()[0] for i in rng]
    return dict(stores=sum(o.startswith(("buffer_store", "global_store")) for o in op),
                loads=sum(o.startswith(("buffer_load", "global_load")) for o in op),
                valu=sum(o.startswith("v_") for o in op),
                f64=sum(bool(re.search(r"_f64($|_)", o)) for o in op),
                dpp=sum("dpp" in i or " wave_sh" in i for i in rng),
                mov64=sum(o == "v_mov_b64" for o in op),
                salu=sum(o.startswith("s_") and o not in ("s_waitcnt", "s_nop") for o in op),
                s_add=sum(o.startswith(("s_add_", "s_addk_")) for o in op),
                s_nop=sum(o == "s_nop" for o in op),
                vmcnt=[int(m.group(1)) for i in rng for m in [re.search(r"vmcnt\((\d+)\)", i)] if m])


def main():
    if sys.argv[1] == "--loops":  # isa_census.py --loops file.s [name-substring ...]: the sweep loops, by instruction class
        ks = kernels(sys.argv[2])
        names = [n for n in ks if any(p in n for p in (sys.argv[3:] or ["k_sor_"]))]
        dm = demangle(names)
        for n in sorted(names, key=lambda n: dm[n]):
            print(dm[n].replace("papof::(anonymous namespace)::", "").replace("void ", "").split("(")[0],
                  "  VGPRs %s  scratch %s B" % (ks[n].get("vgpr", "?"), ks[n].get("scratch", "?")))
            for j, rng in enumerate(loops(ks[n]["text"])):
                c = loop_census(rng)
                print("   loop %d: stores %2d loads %3d VALU %4d (f64 %4d, dpp %3d, v_mov_b64 %2d) scalar %3d (s_add %2d) s_nop %2d"
                      "  vmcnt seq %s" % (j, c["stores"], c["loads"], c["valu"], c["f64"], c["dpp"], c["mov64"], c["salu"],
                                          c["s_add"], c["s_nop"], c["vmcnt"]))
        return
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
