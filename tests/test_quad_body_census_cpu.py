"""Static census of the headline kernel's common RK body on the assembly that was linked (csrc/kernels_fma.phased.s, kept by
csrc/Makefile): the issue slots that compute nothing -- `s_nop` and scalar instructions -- inside the block that holds the
stages of one Dopri5 attempt of the 16-lane integrator (sepaihrd_eval_quad_kernel<0, 1, true, false>, the kernel of bench.py's
default run).  A lone wave pays an issue slot for each of them like for an FP64 instruction."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTING = os.path.join(ROOT, "mathematical-modeling-of-infectious-diseases-v1_amd", "csrc", "kernels_fma.phased.s")
KERNEL = "sepaihrd_eval_quad_kernelILi0ELi1ELb1ELb0EE"

# the same census of the build of commit 3b021d1 ("Test every fp32-arm kernel instantiation and its lane broadcasts"), the
# parent of the change that rearranged the body: 284 instructions, 16 s_nop, 9 scalar, 68 v_fmac_f64_dpp
PARENT_COMMIT = "3b021d1"
PARENT_TOTAL = 284
PARENT_NOP_PLUS_SCALAR = 16 + 9


def body_block(path):
    """the instructions of the label-to-label block of KERNEL with the most v_fmac_f64_dpp"""
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and KERNEL in l and l.split(";")[0].rstrip().endswith(":"))
    blocks, cur = [], []
    for l in lines[start + 1:]:
        t = l.split(";")[0].strip()
        if not t:
            continue
        if t.startswith(".Lfunc_end"):
            break
        if t.startswith(".LBB") and t.endswith(":"):
            blocks.append(cur)
            cur = []
            continue
        if t.startswith(".") or t.endswith(":"):
            continue
        cur.append(t)
    blocks.append(cur)
    return max(blocks, key=lambda b: sum(1 for t in b if t.startswith("v_fmac_f64_dpp")))


def test_common_rk_body_has_fewer_idle_issue_slots_than_the_parent_build():
    assert os.path.exists(LISTING), "kernels_fma.phased.s missing: rebuild (make -C csrc)"
    body = body_block(LISTING)
    fmac_dpp = sum(1 for t in body if t.startswith("v_fmac_f64_dpp"))
    nops = sum(1 for t in body if t.split()[0] == "s_nop")
    scalar = sum(1 for t in body if t.startswith("s_") and t.split()[0] != "s_nop")
    print(f"common RK body: {len(body)} instructions, {fmac_dpp} v_fmac_f64_dpp, {nops} s_nop, {scalar} scalar "
          f"(commit {PARENT_COMMIT}: {PARENT_TOTAL}, 68, 16, 9)")
    assert fmac_dpp == 68, fmac_dpp                      # the block IS the body: the stage sums and contact sums of one attempt
    assert nops + scalar < PARENT_NOP_PLUS_SCALAR, (nops, scalar)
    assert len(body) <= PARENT_TOTAL, len(body)
