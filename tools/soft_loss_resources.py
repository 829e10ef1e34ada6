"""Compare the kernel resource usage of in_batch_loss.hip between two compiles (soft targets added a template argument to the
statistics, lse and gradient kernels; the instantiations that existed must keep their figures).  No GPU.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -Rpass-analysis=kernel-resource-usage -Iinclude \
          twotowermlretrieval_amd/csrc/in_batch_loss.hip -o this.s 2> this.remarks        (and the same over the parent's tree)
    python tools/soft_loss_resources.py parent.remarks this.remarks

An existing instantiation is the SOFT = false one of this build, compared under the parent's name (the parent's kernels lack
the last template argument).  Prints every kernel's figures of both compiles and ends with status 1 if an existing one differs
in VGPRs, AGPRs, scratch, occupancy, spills or LDS.  (SGPRs are printed too; the kernels' argument lists grew.)"""
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from cursor_resources import FIELDS, remarks  # noqa: E402

GATED = tuple(f for f in FIELDS if f != "TotalSGPRs")


def as_parent(name):
    """ib_stats_kernel<G, false> / ib_grad_kernel<G, false> / ib_lse_kernel<false> of this build -> the parent's name (one
    template argument fewer)."""
    m = re.match(r"(ib_(?:stats|grad)_kernel)<(true|false), false>$", name)
    return f"{m.group(1)}<{m.group(2)}>" if m else ("ib_lse_kernel" if name == "ib_lse_kernel<false>" else name)


def is_soft(name):
    return re.match(r"ib_(?:stats|grad)_kernel<(true|false), true>$|ib_lse_kernel<true>$", name) is not None


def main():
    parent, this = remarks(sys.argv[1]), remarks(sys.argv[2])
    new = {n: r for n, r in this.items() if is_soft(n)}
    old = {as_parent(n): r for n, r in this.items() if not is_soft(n)}
    line = lambda r: " ".join(f"{f}={r.get(f)}" for f in FIELDS)
    print(f"kernels: parent {len(parent)} | this build {len(this)} = {len(old)} existing + {len(new)} SOFT")
    missing = sorted(set(parent) - set(old))
    print("parent kernels not found in this build:", missing)
    differ = []
    for n in sorted(parent):
        if n not in old:
            continue
        print(f"  {n}\n     parent: {line(parent[n])}\n     this:   {line(old[n])}")
        if any(parent[n].get(f) != old[n].get(f) for f in GATED):
            differ.append(n)
    print("existing kernels whose VGPR / AGPR / scratch / occupancy / spill / LDS remarks differ:", len(differ), differ)
    print("SOFT instantiations (ib_stats_kernel<GROUPED, SOFT>, ib_grad_kernel<GROUPED, SOFT>, ib_lse_kernel<SOFT>):")
    for n, r in new.items():
        print(f"  {n}\n     this:   {line(r)}")
    return 1 if differ or missing else 0


if __name__ == "__main__":
    sys.exit(main())
