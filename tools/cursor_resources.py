"""Compare the kernel resource usage of score_topk.hip between two compiles, and look inside the tile loop of the AFTER
instantiations (cursor search).  No GPU.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \
          twotowermlretrieval_amd/csrc/score_topk.hip -o this.s 2> this.remarks        (and the same over the parent's tree)
    python tools/cursor_resources.py parent.remarks this.remarks this.s

An existing instantiation is the AFTER = false one of this build, compared under the parent's name (the parent's kernels lack
the last template argument)."""
import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize", "Occupancy", "SGPRs Spill", "VGPRs Spill", "LDS Size")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return [re.sub(r"\(anonymous namespace\)::|void |\(.*$", "", n).strip() for n in out[:len(names)]]


def remarks(path):
    res, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(Function Name|[A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None and m.group(1).strip() in FIELDS:
            cur[m.group(1).strip()] = m.group(2)
    names = list(res)
    return dict(zip(demangle(names), (res[n] for n in names)))


def is_after(name):
    m = re.match(r"(score_topk(16)?_kernel)<(.*)>$", name)
    if not m:
        return False
    args = m.group(3).split(", ")
    return len(args) == (9 if m.group(2) else 10) and args[-1] == "true"


def as_parent(name):
    """score_topk_kernel<..., false> of this build -> the parent's name (one template argument fewer)."""
    m = re.match(r"(score_topk(16)?_kernel)<(.*), false>$", name)
    return f"{m.group(1)}<{m.group(3)}>" if m else name


def tile_loop(asm_path, wanted):
    """Per AFTER kernel: scratch accesses and s_waitcnt vmcnt(0) between the first and the last MFMA of its text."""
    out, name, body = {}, None, []
    mangled = {}
    for line in open(asm_path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m:
            name, body = m.group(1), []
            mangled[name] = body
        elif name is not None:
            body.append(line)
            if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
                name = None
    names = list(mangled)
    for nice, raw in zip(demangle(names), names):
        if nice not in wanted:
            continue
        ins = [l.strip() for l in mangled[raw] if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        mf = [i for i, l in enumerate(ins) if l.startswith("v_mfma")]
        first, last = mf[0], mf[-1]
        scr = lambda seg: sum(1 for l in seg if l.startswith(("scratch_", "buffer_load", "buffer_store")))
        out[nice] = (scr(ins[:first]), scr(ins[first:last + 1]), scr(ins[last + 1:]),
                     sum(1 for l in ins[first:last + 1] if re.match(r"s_waitcnt vmcnt\(0\)", l)), len(mf))
    return out


def main():
    parent, this = remarks(sys.argv[1]), remarks(sys.argv[2])
    new = {n: r for n, r in this.items() if is_after(n)}
    old = {as_parent(n): r for n, r in this.items() if not is_after(n)}
    print(f"kernels: parent {len(parent)} | this build {len(this)} = {len(old)} existing + {len(new)} AFTER")
    print("parent kernels not found in this build:", sorted(set(parent) - set(old)))
    differ = sorted(n for n in parent if n in old and parent[n] != old[n])
    print("existing kernels whose SGPR / VGPR / AGPR / scratch / occupancy / spill / LDS remarks differ:", len(differ), differ)
    print("AFTER instantiations (score_topk_kernel<NS, CAP, MAXONLY, NT, BF, MASKED, COUNT, TAGGED, BIASED, AFTER>, "
          "score_topk16_kernel<NS, CAP, MAXONLY, NT, MASKED, COUNT, TAGGED, BIASED, AFTER>):")
    for n, r in new.items():
        print("  ", n, " ".join(f"{f}={r.get(f)}" for f in FIELDS[:-1]))
    if len(sys.argv) > 3:
        loops = tile_loop(sys.argv[3], set(new))
        print(f"disassembly of the {len(loops)} AFTER instantiations: scratch accesses before the first MFMA / between the first "
              "and the last MFMA / behind the last; s_waitcnt vmcnt(0) between the first and the last MFMA")
        for n, (a, b, c, w, nm) in loops.items():
            print(f"   {n}: scratch {a} / {b} / {c}; vmcnt(0) {w}; MFMAs {nm}")
        print("AFTER instantiations with scratch or vmcnt(0) inside the tile loop:", sum(1 for v in loops.values() if v[1] or v[3]))


if __name__ == "__main__":
    main()
