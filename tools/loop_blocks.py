"""tools/loop_blocks.py OBJECT.o KERNEL-SUBSTRING [LABEL]
Per-block instruction table of the every-step path of a headline beam kernel's time loop (csrc/beam_wave_step.inc, the HL
family), from the gfx950 disassembly of a hipcc object file; no GPU needed.  With tools/isa_table.sh it makes
profiles/TAG_isa_table.txt.

The time loop is the backward scalar branch with the shortest body that holds, in this order, the step's push
(ds_permute_b32), its key write (ds_write2st64_b32 of the two key words, or -- r17: the raw probability word alone --
ds_write_b32), the count's own term (v_mul_f32 by 2^100, r17: by -2^100) and its division (v_div_fixup_f32).
The every-step path is its body in address order, minus what a FORWARD scalar branch inside the body jumps over when its
target is inside the body as well: the row-FIFO rotation (one step in six) and the inline block that ends a failing read.
Forward branches that leave the body (the rare blocks behind the loop) are counted as not taken, exec branches
(s_cbranch_execz / execnz) and the unconditional s_branch of their else paths as falling through: the instructions of every
exec region are counted once, in address order.

Blocks, by landmarks in address order (the scheduler moves single instructions across them: the totals are exact, the
split is as good as the landmarks):
  extension + push          loop head .. the second ds_permute_b32
  key + table write         .. the ds_write2st64_b32 of the two key words (r17: the ds_write_b32 of the raw probability word)
  numbering + record stores .. the instruction in front of the count's own term (v_mul_f32 by 2^100 or -2^100)
  rank                      .. the add behind the last v_fma_f32 ... clamp
  end-of-read test          .. the instruction in front of v_cvt_i32_f32 (the rank as an integer)
  survivor table            .. the last ds_bpermute_b32 between the table's ds_write2_b32 and the eviction's
                               global_store_dword (up to r17 the second of two look-ups, `fate` and `own`; r18: `fate`, the only
                               one left -- the same instructions fall into the same blocks on both)
  child fate + eviction     .. the s_or_b64 exec behind the eviction's global_store_dword
  gather + division         .. the last ds_bpermute_b32 in front of the kind field's v_and_b32 ..., 3, ...
  rare-branch vote          .. the scalar branch to the rare block
  commit                    .. the loop's backward branch
A last line counts the forms priced one by one in profiles/r15a_issue_cost.txt: selects on VCC, 64-bit vector shifts and moves,
scalar branches that are TAKEN on the every-step path (the forward branches it jumps with), and the rotation path -- its length
and its integer multiplies -- wherever the compiler put it (skipped inline, or behind the loop).  LOOP_DUMP=file writes the
every-step path and the blocks off it as text.
Classes (profiles/r12a_issue_cost.txt, r14a_issue_cost.txt, six wavefronts per SIMD): cheap VALU = plain f32 arithmetic and
32-bit add / sub / logic / move, about 1.2 - 1.4 ns; expensive VALU = every other vector ALU instruction (compares into a
scalar pair, selects, shifts, carry forms, three-operand integer forms, conversions, the division's special forms), about
1.9 - 2.1 ns.  SALU excludes branches, waits and no-ops."""
import re
import subprocess
import sys
import tempfile

B = "/opt/rocm/lib/llvm/bin"
KEY_WRITES = ("ds_write2st64_b32", "ds_write_b32")  # two key words (up to r16) / the raw probability word alone (r17)
OWN_TERMS = ("0x71800000", "0xf1800000")            # the literal of the count's own term: 2^100 / -2^100
CHEAP = {"v_add_f32", "v_sub_f32", "v_subrev_f32", "v_mul_f32", "v_fma_f32", "v_fmac_f32", "v_mac_f32", "v_add_u32", "v_sub_u32",
         "v_subrev_u32", "v_and_b32", "v_or_b32", "v_xor_b32", "v_not_b32", "v_mov_b32"}
BLOCKS = ["extension + push", "key + table write", "numbering + record stores", "rank", "end-of-read test", "survivor table",
          "child fate + eviction", "gather + division", "rare-branch vote", "commit"]


def disasm(obj):
    t = tempfile.mkdtemp()
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, t + "/f.bin"])
    subprocess.check_call([B + "/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + t + "/f.bin", "--output=" + t + "/d.co", "--unbundle"])
    return subprocess.check_output([B + "/llvm-objdump", "-d", t + "/d.co"]).decode()


def kernel(text, pat):
    m = [x for x in re.finditer(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^\n|\Z)", text, re.S | re.M) if pat in x.group(1)]
    assert len(m) == 1, [x.group(1) for x in m]
    ins = []
    for l in m[0].group(2).splitlines():
        mm = re.match(r"\s+(\S+)\s*(.*?)\s*//\s*([0-9A-F]+):", l)
        if mm:
            ins.append((int(mm.group(3), 16), mm.group(1), mm.group(2)))
    return ins


def target(addr, args):
    off = int(args.split()[-1])
    return addr + 4 + (off - 65536 if off >= 32768 else off) * 4


def every_step_path(ins):
    loops = []
    for addr, op, args in ins:
        if op in ("s_cbranch_scc0", "s_cbranch_scc1", "s_branch") and target(addr, args) <= addr:
            body = [x for x in ins if target(addr, args) <= x[0] <= addr]
            marks = []  # the step's landmarks must appear in the step's order (a rare block that jumps back into the loop fails this)
            for want in (("ds_permute_b32",), KEY_WRITES, OWN_TERMS, ("v_div_fixup_f32",)):
                start = marks[-1] + 1 if marks else 0
                hit = next((j for j in range(start, len(body)) if body[j][1] in want or any(w in body[j][2] for w in want)), None)
                if hit is None:
                    break
                marks.append(hit)
            if len(marks) == 4:
                loops.append(body)
    body = min(loops, key=len)
    lo, hi = body[0][0], body[-1][0]
    path, skip_to = [], None
    skipped = []  # what each taken forward branch jumps over, in address order
    outside = []
    for addr, op, args in body:
        if skip_to is not None:
            if addr < skip_to:
                skipped[-1].append((addr, op, args))
                continue
            skip_to = None
        path.append((addr, op, args))
        if op in ("s_cbranch_scc0", "s_cbranch_scc1") and addr != hi:
            t = target(addr, args)
            if addr < t <= hi:
                skip_to = t
                skipped.append([])
            elif t > hi:
                # a block behind the loop that comes back into it (an unlikely block moved out of line): not on the every-step
                # path and not a taken branch, but listed, so that the rotation path is found wherever it was placed
                out = []
                for x in ins:
                    if x[0] < t:
                        continue
                    out.append(x)
                    if x[1] == "s_branch":
                        if lo <= target(x[0], x[2]) <= hi:
                            outside.append(out)
                        break
                    if x[1] == "s_endpgm" or len(out) > 400:
                        break
    return path, skipped, outside


def split(path):
    ops = [re.sub(r"_(e32|e64)$", "", op) for _, op, _ in path]
    txt = [op + " " + args for _, op, args in path]

    def first(pred, start=0):
        return next(i for i in range(start, len(path)) if pred(i))

    def last(pred, end):
        return max(i for i in range(end) if pred(i))

    e = []
    p1 = first(lambda i: ops[i] == "ds_permute_b32")
    e.append(first(lambda i: ops[i] == "ds_permute_b32", p1 + 1))
    e.append(first(lambda i: ops[i] in KEY_WRITES, e[-1]))
    e.append(first(lambda i: ops[i] == "v_mul_f32" and any(w in txt[i] for w in OWN_TERMS), e[-1]) - 1)
    lf = last(lambda i: ops[i] == "v_fma_f32" and "clamp" in txt[i], len(path))
    e.append(first(lambda i: ops[i] == "v_add_f32", lf))
    cvt = first(lambda i: ops[i] == "v_cvt_i32_f32", e[-1])
    e.append(cvt - 1)
    w2 = first(lambda i: ops[i] == "ds_write2_b32", cvt)
    st = first(lambda i: ops[i] == "global_store_dword", w2)
    e.append(last(lambda i: ops[i] == "ds_bpermute_b32", st))
    assert e[-1] > w2, "no look-up between the table's write and the eviction store"
    e.append(first(lambda i: ops[i] == "s_or_b64" and "exec" in txt[i], st))
    kind = first(lambda i: ops[i] == "v_and_b32" and re.search(r", 3, v\d+$", txt[i]), e[-1])
    lastperm = max(i for i in range(len(path)) if ops[i] == "ds_bpermute_b32" and i < first(
        lambda j: ops[j] in ("s_cbranch_scc0", "s_cbranch_scc1"), kind))
    e.append(max(lastperm, e[-1] + 1))
    e.append(first(lambda i: ops[i] in ("s_cbranch_scc0", "s_cbranch_scc1"), kind))
    e.append(len(path) - 1)
    return e


def classify(op):
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    if op in ("s_waitcnt", "s_nop"):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith("v_"):
        base = re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)
        return "cheap" if base in CHEAP else "exp"
    return "other"


def main():
    obj, pat = sys.argv[1], sys.argv[2]
    label = sys.argv[3] if len(sys.argv) > 3 else pat
    path, skipped, outside = every_step_path(kernel(disasm(obj), pat))
    ends = split(path)
    cols = ["cheap", "exp", "salu", "lds", "vmem", "saveexec", "branch", "all"]
    print("# %s: every-step path of the time loop, %d instructions" % (label, len(path)))
    print("%-28s | cheap VALU | expensive VALU | SALU | LDS | VMEM | saveexec regions | branches | all" % "block")
    tot = dict.fromkeys(cols, 0)
    start = 0
    for name, end in zip(BLOCKS, ends):
        row = dict.fromkeys(cols, 0)
        for _, op, _ in path[start:end + 1]:
            c = classify(op)
            if c in row:
                row[c] += 1
            if op.startswith("s_and_saveexec") or op.startswith("s_or_saveexec"):
                row["saveexec"] += 1
            row["all"] += 1
        print("%-28s | %10d | %14d | %4d | %3d | %4d | %16d | %8d | %3d" % ((name,) + tuple(row[c] for c in cols)))
        for c in cols:
            tot[c] += row[c]
        start = end + 1
    print("%-28s | %10d | %14d | %4d | %3d | %4d | %16d | %8d | %3d" % (("whole path",) + tuple(tot[c] for c in cols)))
    txt = [(op, args) for _, op, args in path]
    v01 = [i for i, (op, a) in enumerate(txt) if op.startswith("v_cndmask_b32") and re.match(r"v\d+, 0, 1, ", a)]
    round_trips = 0
    for i in v01:
        dst = txt[i][1].split(",")[0]
        for op, a in txt[i + 1:i + 12]:
            if op.startswith("v_cmp_ne_u32") and re.search(r", 0, %s$" % dst, a):
                round_trips += 1
                break
            if a.split(",")[0] == dst:  # the register is written again (the pushed 0 / 1 word is data: ds_permute's result)
                break
    print("# v_cndmask 0, 1: %d, of them read only by a compare with 0 (a vote through a vector register): %d;"
          " 64-bit vector compares: %d; s_mov of a 32-bit literal: %d" % (
              len(v01), round_trips, sum(re.match(r"v_cmp\w*_[uif]64", op) is not None for op, _ in txt),
              sum(op == "s_mov_b32" and re.search(r"0x[0-9a-f]{5,}", a) is not None for op, a in txt)))
    print("# VALU %d (cheap %d + expensive %d), SALU %d" % (tot["cheap"] + tot["exp"], tot["cheap"], tot["exp"], tot["salu"]))
    # Forms priced one by one in profiles/r15a_issue_cost.txt.  A VCC-form select: v_cndmask_b32 in its e32 / dpp / sdwa encoding
    # (the mask is VCC by encoding) or an e64 whose pair operand is spelled vcc.  The rotation path: what the taken forward
    # branch in front of the row FIFO's refill jumps over (the skipped region that holds the refill's global_load), or the
    # block behind the loop that holds it when the rotation was moved out of line.
    base = lambda op: re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)
    vcc_sel = sum(base(op) == "v_cndmask_b32" and (not op.endswith("_e64") or a.rstrip().endswith("vcc")) for op, a in txt)
    wide = sum(re.match(r"v_(lshrrev|lshlrev|ashrrev|mov)_b64|v_ashrrev_i64", base(op)) is not None for op, _ in txt)
    rot = next((r for r in skipped + outside if any(op.startswith(("global_load", "flat_load")) for _, op, _ in r)), [])
    muls = sum(re.match(r"v_(mul_lo_u32|mul_hi_[ui]32|mad_[ui]64_[ui]32|mul_[ui]32_[ui]24|mad_[ui]32_[ui]24)", op) is not None
               for _, op, _ in rot)
    print("# VCC-form selects: %d; 64-bit vector shifts and moves: %d; taken scalar branches: %d;"
          " rotation path: %d instructions, integer multiplies on it: %d" % (vcc_sel, wide, len(skipped), len(rot), muls))
    import os
    if os.environ.get("LOOP_DUMP"):  # the two paths as text, for reading next to the source
        with open(os.environ["LOOP_DUMP"], "w") as f:
            for a, op, ar in path:
                f.write("%6x  %s %s\n" % (a, op, ar))
            for r in skipped + outside:
                f.write("---- jumped over / out of line ----\n")
                for a, op, ar in r:
                    f.write("%6x  %s %s\n" % (a, op, ar))


main()
