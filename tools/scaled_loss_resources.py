"""Compare the kernel resource usage of in_batch_loss.hip between two compiles (the device-resident logit scale added kernels
of its own beside the existing ones -- ib_prep_ls_kernel, ib_stats_ls_kernel<..>, ib_grad_ls_kernel<..>, ib_project_dots_kernel --
and moved the bodies of ib_prep_kernel and ib_project_kernel into functions they share with the new ones; every kernel that
existed must keep its figures).  No GPU.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -Rpass-analysis=kernel-resource-usage -Iinclude \
          twotowermlretrieval_amd/csrc/in_batch_loss.hip -o this.s 2> this.remarks        (and the same over the parent's tree)
    python tools/scaled_loss_resources.py parent.remarks this.remarks

The existing kernels keep their names and argument lists, so they are compared name by name, SGPRs included.  Prints every
kernel's figures of both compiles and ends with status 1 if an existing one is missing or differs in SGPRs, VGPRs, AGPRs,
scratch, occupancy, spills or LDS, or if a new one uses scratch."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from cursor_resources import FIELDS, remarks  # noqa: E402


def main():
    parent, this = remarks(sys.argv[1]), remarks(sys.argv[2])
    new = {n: r for n, r in this.items() if n not in parent}
    line = lambda r: " ".join(f"{f}={r.get(f)}" for f in FIELDS)  # noqa: E731
    print(f"kernels: parent {len(parent)} | this build {len(this)} = {len(this) - len(new)} existing + {len(new)} new")
    missing = sorted(set(parent) - set(this))
    print("parent kernels not found in this build:", missing)
    differ = []
    for n in sorted(parent):
        if n not in this:
            continue
        print(f"  {n}\n     parent: {line(parent[n])}\n     this:   {line(this[n])}")
        if any(parent[n].get(f) != this[n].get(f) for f in FIELDS):
            differ.append(n)
    print("existing kernels whose SGPR / VGPR / AGPR / scratch / occupancy / spill / LDS remarks differ:", len(differ), differ)
    print("new kernels:")
    for n, r in sorted(new.items()):
        print(f"  {n}\n     this:   {line(r)}")
    scratch = sorted(n for n, r in new.items() if r.get("ScratchSize") != "0" or r.get("VGPRs Spill") != "0")
    print("new kernels that use scratch or spill VGPRs:", len(scratch), scratch)
    return 1 if differ or missing or scratch else 0


if __name__ == "__main__":
    sys.exit(main())
