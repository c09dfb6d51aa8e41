"""Device code of two trees, kernel by kernel (no GPU needed).

  python tools/isa_compare.py dump <dir>                     device assembly of every build.py SOURCES entry of THIS tree
  python tools/isa_compare.py compare <parent dir> <dir> [--out FILE]

`dump` runs hipcc with the flags build.py uses for the file plus `--cuda-device-only -S`.  `compare` splits each dump per
kernel symbol (the mangled name: a kernel may have moved to another file) and compares, per kernel,
  - the resource figures: VGPR / AGPR / SGPR counts, spills, scratch, LDS (the .amdgpu_metadata record) and the occupancy
    the assembler prints;
  - the `.amdhsa_kernel` block and the instruction text.
What depends on a kernel's place in its translation unit, not on the kernel, is normalised first: the function ordinal in
local labels (.LBB<f>_<n> and the loop comments naming them, .Lfunc_begin<f>, .Lfunc_end<f>), the column a comment starts in,
and the compilation-unit symbol __hip_cuid_<hex>.
Exit status 1 when a kernel of the parent is missing or any resource figure differs."""
import difflib
import importlib.util
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = [".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
           ".private_segment_fixed_size", ".group_segment_fixed_size"]


def _build_recipe():
    spec = importlib.util.spec_from_file_location("fs_build", os.path.join(ROOT, "gpu-fluid-simulation_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def dump(outdir):
    b = _build_recipe()
    os.makedirs(outdir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    procs = []
    for src in b.SOURCES:
        sp = os.path.join(b.CSRC, src)
        cmd = [hipcc] + b._flags(sp) + ["--cuda-device-only", "-S", sp, "-o", os.path.join(outdir, src.replace(".hip", ".s"))]
        procs.append((src, subprocess.Popen(cmd)))
    for src, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {src}")


def _normalise(line):
    line = re.sub(r"(\.L|\b)BB\d+_", r"\1BB_", line)                      # labels and the loop comments that name them
    line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
    line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", line)
    return re.sub(r"\s+", " ", line).strip()                      # comment columns move with a label's width


def kernels_of(path):
    """{symbol: {"file", "text", "desc", "figures"}} of one assembly file."""
    lines = open(path).read().split("\n")
    name = os.path.basename(path).replace(".s", ".hip")
    names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    out = {k: {"file": name, "text": None, "desc": None, "figures": {}} for k in names}
    i = 0
    while i < len(lines):
        l = lines[i]
        m = re.match(r"(\S+):\s*(;.*)?$", l)
        if m and m.group(1) in out and out[m.group(1)]["text"] is None:
            k, j = m.group(1), i + 1
            while not re.match(r"\.Lfunc_end\d+:", lines[j]):
                j += 1
            out[k]["text"] = [_normalise(x) for x in lines[i + 1:j]]      # (holds the kernel's descriptor block too)
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            k, j = m.group(1), i + 1
            while ".end_amdhsa_kernel" not in lines[j]:
                j += 1
            out[k]["desc"] = [x.strip() for x in lines[i + 1:j]]
            # the assembler's summary of the kernel follows its descriptor
            while not lines[j].startswith("; Occupancy:"):
                j += 1
            out[k]["figures"]["occupancy"] = int(lines[j].split(":")[1])
            i = j
        i += 1
    # .amdgpu_metadata: one record per kernel, `.name:` among its keys
    rec = {}
    for l in lines:
        m = re.match(r"\s*(?:- )?(\.[a-z_]+):\s*(\S+)\s*$", l)
        if not m:
            continue
        if l.startswith("  - ."):                                         # a new kernel record (the outer list's item)
            rec = {}
        rec[m.group(1)] = m.group(2)
        if m.group(1) == ".name" and m.group(2) in out:
            out[m.group(2)]["_rec"] = rec
    for k, v in out.items():
        r = v.pop("_rec")
        for f in FIGURES:
            v["figures"][f.lstrip(".")] = int(r[f])
        assert v["text"] is not None and v["desc"] is not None, k
    return out


def kernels_in(d):
    all_k = {}
    for f in sorted(os.listdir(d)):
        if f.endswith(".s"):
            for k, v in kernels_of(os.path.join(d, f)).items():
                assert k not in all_k, f"{k} defined twice"
                all_k[k] = v
    return all_k


def _demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
        # `fsd::k_force<0, false, false>`: the parameter list adds nothing (no kernel name is overloaded)
        return {n: re.sub(r"^(?:void )?([^(]+)\(.*$", r"\1", o) for n, o in zip(names, out)}
    except OSError:
        return {n: n for n in names}


def compare(da, db, out_path):
    A, B = kernels_in(da), kernels_in(db)
    pretty = _demangle(sorted(set(A) | set(B)))
    rows, bad = [], 0
    n_same_fig = n_same_text = 0
    for k in sorted(A, key=lambda s: (B.get(s, A[s])["file"], pretty[s])):
        a, b = A[k], B.get(k)
        if b is None:
            rows.append(f"MISSING: {a['file']}: {pretty[k]}")
            bad += 1
            continue
        fig = a["figures"] == b["figures"]
        text = a["text"] == b["text"] and a["desc"] == b["desc"]
        n_same_fig += fig
        n_same_text += text
        bad += not fig
        where = b["file"] if a["file"] == b["file"] else f"{b['file']} (was {a['file']})"
        if not text:          # how far apart: lines of one side without a partner in the other
            sm = difflib.SequenceMatcher(None, a["text"], b["text"], autojunk=False)
            moved = max(len(a["text"]), len(b["text"])) - sum(m.size for m in sm.get_matching_blocks())
        stream = "identical" if text else f"DIFFERENT ({moved} of {len(b['text'])} lines)"
        rows.append(f"{'same' if fig else 'DIFFER'} figures, {stream} stream: {where}: {pretty[k]} {b['figures']}"
                    + ("" if fig else f" parent {a['figures']}"))
    for k in sorted(set(B) - set(A)):
        rows.append(f"NEW: {B[k]['file']}: {pretty[k]} {B[k]['figures']}")
    head = [f"{len(A)} kernels of the parent: {n_same_fig} identical in VGPR/AGPR/SGPR/spills/scratch/LDS/occupancy, "
            f"{len(A) - n_same_fig - sum(k not in B for k in A)} differ, {sum(k not in B for k in A)} missing; "
            f"{n_same_text} with identical instruction stream and .amdhsa_kernel block, {len(set(B) - set(A))} new"]
    per_file = {}
    for k, b in B.items():
        per_file[b["file"]] = per_file.get(b["file"], 0) + 1
    head.append("kernels per file: " + ", ".join(f"{f} {n}" for f, n in sorted(per_file.items())))
    text = "\n".join(head + rows) + "\n"
    if out_path:
        with open(out_path, "a") as f:
            f.write(text)
    sys.stdout.write(text if not out_path else "\n".join(head) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None))
    else:
        sys.exit(__doc__)
