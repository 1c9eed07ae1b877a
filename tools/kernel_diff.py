"""Per-kernel comparison of two builds of the library's objects (hnsw_amd/csrc/obj
of two trees built with the same flags): for every gfx950 kernel symbol the
instruction count, VGPRs, SGPRs, static LDS and scratch from the code object's
metadata, and whether the disassembly (addresses and encodings stripped) is
identical.  The record of a change that must leave the existing kernels as they
were (profiles/filtered_search_build.txt).  Objects are paired by file name;
with --pool the kernels of every object of each directory go into one table and
are paired by symbol, for a change that moves kernels between objects
(profiles/build_refactor.txt); symbols found on one side only are listed.
Usage: python tools/kernel_diff.py [--pool] PARENT_OBJ_DIR BRANCH_OBJ_DIR [unit-glob]"""
import collections
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


class HostOnly(Exception):
    """the object holds no device code (no .hip_fatbin section)"""


def code_object(obj, tmp):
    """the gfx950 code object of a HIP object file (its .hip_fatbin bundle);
    any tool failure other than a missing bundle ends the run"""
    fat = os.path.join(tmp, os.path.basename(obj) + ".fatbin")
    out = os.path.join(tmp, os.path.basename(obj) + ".co")
    sections = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-S", "--wide", obj], capture_output=True,
                              text=True, check=True).stdout
    if ".hip_fatbin" not in sections:
        raise HostOnly(obj)
    # (with an output named: llvm-objcopy otherwise rewrites the object in place, which make then takes for new)
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, fat + ".o"],
                          stderr=subprocess.DEVNULL)
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=" + TARGET,
                           "--input=" + fat, "--output=" + out, "--unbundle"], stderr=subprocess.DEVNULL)
    return out


def kernels(co):
    """symbol -> (instructions as text, metadata dict)"""
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                         capture_output=True, text=True, check=True).stdout
    body, cur = collections.defaultdict(list), None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]* ?<([^>]+)>:$", line.strip())
        if m:
            cur = m.group(1)
            continue
        t = line.strip()
        if cur and t and not t.startswith("//") and t != "...":  # ("...": zero padding after the kernel's code)
            t = re.sub(r"\s*//.*$", "", t)        # (the address comment)
            t = re.sub(r"<[^>]*>", "<L>", t)      # (branch targets by label text)
            body[cur].append(t)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True,
                           check=True).stdout
    # (a kernel's entry lists its keys in alphabetical order: .agpr_count opens it)
    entries, cur_m = [], None
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2).strip()
        if key == "agpr_count":
            cur_m = {}
            entries.append(cur_m)
        if cur_m is None:
            continue
        if key in ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                   "vgpr_spill_count", "sgpr_spill_count"):
            cur_m[key] = int(val)
        elif key == "symbol":
            cur_m["symbol"] = val.strip("'\"")[:-3]  # (without .kd)
    meta = {e.pop("symbol"): e for e in entries if "symbol" in e}
    return {k: (v, meta.get(k, {})) for k, v in body.items() if k in meta}


def template_of(sym):
    m = re.search(r"(k_[a-z0-9_]+)", sym)
    return m.group(1) if m else sym


def compare(name, ka, kb, tot, per, list_single=False):
    """count the kernels of two symbol tables, print the differing ones (and,
    list_single, the symbols found on one side only)"""
    for s in sorted(set(ka) | set(kb)):
        t = template_of(s)
        if s not in ka or s not in kb:
            side = "only parent" if s in ka else "only branch"
            per[t][side] += 1
            tot[side] += 1
            if list_single:
                print(f"{side.upper()} {name} {s}")
            continue
        per[t]["kernels"] += 1
        tot["kernels"] += 1
        if ka[s] != kb[s]:
            per[t]["differing"] += 1
            tot["differing"] += 1
            print(f"DIFF {name} {s}: instructions {len(ka[s][0])} -> {len(kb[s][0])}, metadata {ka[s][1]} -> {kb[s][1]}")
        if ka[s][1].get("private_segment_fixed_size", 0) or kb[s][1].get("private_segment_fixed_size", 0):
            tot["with scratch"] += 1


def pool(obj_dir, pat, tmp):
    """the kernels of every object of a directory in one table; a symbol that
    two objects hold must be the same kernel in both"""
    out = {}
    for p in sorted(glob.glob(os.path.join(obj_dir, pat))):
        try:
            ks = kernels(code_object(p, tmp))
        except HostOnly:
            continue
        for s, k in ks.items():
            if s in out and out[s] != k:
                sys.exit(f"{obj_dir}: {s} differs between two objects (one of them {os.path.basename(p)})")
            out[s] = k
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--pool"]
    pooled = len(args) != len(sys.argv) - 1
    a_dir, b_dir = args[0], args[1]
    pat = args[2] if len(args) > 2 else "*.o"
    tot = collections.Counter()
    per = collections.defaultdict(collections.Counter)
    with tempfile.TemporaryDirectory() as tmp:
        if pooled:
            ka, kb = pool(a_dir, pat, tmp), pool(b_dir, pat, tmp)
            print(f"kernels: parent {len(ka)}, branch {len(kb)}")
            compare("(pooled)", ka, kb, tot, per, list_single=True)
        else:
            units = sorted(os.path.basename(p) for p in glob.glob(os.path.join(a_dir, pat)))
            for u in units:
                if not os.path.exists(os.path.join(b_dir, u)):
                    print(f"{u}: only in parent")
                    continue
                try:
                    compare(u, kernels(code_object(os.path.join(a_dir, u), tmp)),
                            kernels(code_object(os.path.join(b_dir, u), tmp)), tot, per)
                except HostOnly:
                    continue
            for u in sorted(os.path.basename(p) for p in glob.glob(os.path.join(b_dir, pat))):
                if u not in units:
                    try:
                        kb = kernels(code_object(os.path.join(b_dir, u), tmp))
                    except HostOnly:
                        continue
                    tot["new"] += len(kb)
                    print(f"{u}: only in branch, {len(kb)} kernels")
                    for s, (ins, md) in sorted(kb.items()):
                        print(f"  NEW {s}: {len(ins)} instructions, {md}")
    print(f"compared {tot['kernels']} kernels: identical ISA and metadata {tot['kernels'] - tot['differing']}, "
          f"differing {tot['differing']}; kernels with scratch > 0 (either side): {tot['with scratch']}")
    if pooled:
        print(f"symbols only in parent {tot['only parent']}, only in branch {tot['only branch']}")
    print("per kernel template: kernels / differing")
    for t in sorted(per):
        extra = "".join(f", {k} {v}" for k, v in per[t].items() if k.startswith("only"))
        print(f"  {t}: {per[t]['kernels']} / {per[t]['differing']}{extra}")
    if tot["kernels"] + tot["new"] == 0:
        sys.exit("no kernel was compared: wrong directories, unit pattern or target?")


if __name__ == "__main__":
    main()
