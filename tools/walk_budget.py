"""Instruction budget of the 2D force walk, its scan and the density row loop, read from the device assembly (no GPU needed).

  python tools/walk_budget.py [--keep DIR]

Compiles kernels_force.hip and kernels_density.hip to assembly with the flags build.py uses for them (plus
`--cuda-device-only -S`, as tools/isa_compare.py does) and prints, for k_force<0,false,false>, k_density<false,true> and
k_force_quad<0,false,false>: VGPRs, SGPRs, scratch and LDS, and the VALU instructions of the hot loops per unit of work.  A loop is
the set of basic blocks the assembler's comments attribute to one inner loop header; loops are told apart by what they hold:
  walk     the loop with the transcendentals (v_rsq_f32): VALU per neighbour = VALU of the loop / number of v_rsq_f32
           (one per unrolled body; terms, accumulate, fetch, queue refill and loop control all counted);
  scan     a loop with add-with-carry (v_addc_co_u32, one per candidate): VALU per trip of four = 4 * VALU / number of them;
  density  a loop with ds_read2_b64 and no add-with-carry (two reads = four candidates): VALU per trip = 2 * VALU / reads.
A report, not a test: it looks for nothing but these counts.  profiles/walk_diet_isa.txt holds its output for two trees."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_compare as I  # noqa: E402

UNITS = ("kernels_force.hip", "kernels_density.hip")
KERNELS = ("fsd::k_force<0, false, false>", "fsd::k_density<false, true>", "fsd::k_force_quad<0, false, false>")


def assemble(outdir):
    b = I._build_recipe()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    procs = []
    for src in UNITS:
        sp = os.path.join(b.CSRC, src)
        cmd = [hipcc] + b._flags(sp) + ["--cuda-device-only", "-S", sp, "-o", os.path.join(outdir, src.replace(".hip", ".s"))]
        procs.append((src, subprocess.Popen(cmd, stderr=subprocess.DEVNULL)))
    for src, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {src}")


def loops_of(text):
    """{header label: [opcodes]} of the inner loops of one kernel (isa_compare's normalised text).  The assembler's comments name the
    blocks of every natural loop; where a loop is entered in the middle of its first body (the walk: the compiler lets the first trip
    begin at the terms, behind the header), the blocks in front of the header belong to no natural loop and carry no comment.  So a
    loop is taken as the cycle through its header over the blocks that name this header or none."""
    ops, note_of, label_at, headers = [], [], {}, []
    cur = label = None
    for line in text:
        m = re.match(r"(?:\.L(BB_\d+):|; %bb\.\d+:)\s*(?:;\s*(.*))?$", line)
        if m:                                   # a basic block starts: which loop does the comment put it in?
            note, label = m.group(2) or "", m.group(1)
            h = re.search(r"in Loop: Header=(BB_\d+)", note)
            cur = h.group(1) if h else None
            if label:
                label_at[label] = len(ops)
        if label and "This Inner Loop Header" in line:      # on the label's line, or (a nested loop) on a comment line below it
            cur = label
            headers.append(label)
        if m:
            continue
        if line and not line.startswith((";", ".")):
            ops.append(line.split())
            note_of.append(cur)
            label = None
    succ = [[] for _ in ops]
    for i, o in enumerate(ops):
        if o[0].startswith(("s_cbranch", "s_branch")) and o[-1].startswith(".L"):
            succ[i].append(label_at[o[-1][2:]])
        if o[0] not in ("s_branch", "s_endpgm") and i + 1 < len(ops):
            succ[i].append(i + 1)
    pred = [[] for _ in ops]
    for i, ss in enumerate(succ):
        for s in ss:
            pred[s].append(i)

    def reach(start, edges, ok):
        seen, todo = {start}, [start]
        while todo:
            for j in edges[todo.pop()]:
                if j not in seen and ok(j):
                    seen.add(j)
                    todo.append(j)
        return seen

    loops = {}
    for h in headers:
        ok = lambda j, h=h: note_of[j] in (h, None)
        cyc = reach(label_at[h], succ, ok) & reach(label_at[h], pred, ok)
        loops[h] = [ops[i][0] for i in sorted(cyc)]
    return loops


def is_valu(op):
    return op.startswith("v_")


def report(kernel, rec, out):
    f = rec["figures"]
    out.append(f"{kernel}: {f['vgpr_count']} VGPRs, {f['sgpr_count']} SGPRs, scratch {f['private_segment_fixed_size']} B, "
               f"LDS {f['group_segment_fixed_size']} B, occupancy {f['occupancy']}")
    for head, ops in loops_of(rec["text"]).items():
        valu = sum(is_valu(o) for o in ops)
        rsq, addc = ops.count("v_rsq_f32_e32"), ops.count("v_addc_co_u32")
        rd2 = ops.count("ds_read2_b64")
        if rsq:
            out.append(f"    walk loop {head}: {valu} VALU, {rsq} bodies: {valu / rsq:.1f} VALU per neighbour")
        elif addc:
            out.append(f"    scan loop {head}: {valu} VALU, {addc} candidates: {4 * valu / addc:.1f} VALU per trip of four")
        elif rd2:
            out.append(f"    density row loop {head}: {valu} VALU, {rd2} ds_read2_b64: {2 * valu / rd2:.1f} VALU per trip of four")


def main():
    keep = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else None
    with tempfile.TemporaryDirectory() as tmp:
        d = keep or tmp
        os.makedirs(d, exist_ok=True)
        assemble(d)
        K = {}
        for u in UNITS:
            K.update(I.kernels_of(os.path.join(d, u.replace(".hip", ".s"))))
    pretty = I._demangle(sorted(K))
    out = []
    for want in KERNELS:
        hit = [k for k in K if pretty[k] == want]
        if not hit:
            out.append(f"{want}: not found")
            continue
        report(want, K[hit[0]], out)
    print("\n".join(out))


if __name__ == "__main__":
    main()
