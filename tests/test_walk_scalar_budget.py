"""What the plain walk's loop pays beside its vector instructions, read from the device assembly (build/kernels.s, which
tests/test_kernel_resources.py makes): scalar ALU instructions and branches inside the walk loop of the bench line's kernel,
k_trace<primary, BLAS, reciprocal arithmetic>.  The kernel is bound by instruction issue; a scalar instruction costs a third
of a vector one there and a taken branch more than two (profiles/r02_ubench_issue_rates.log), and the source forms that keep
the loop's layout ("what the compiler must not undo") are easy to lose: a wave-uniform if / else whose
arms hold per-lane branches, a ballot of a combined condition, a flag the compiler can trace - each comes back as a dozen
scalar instructions and a few branches.  The bounds are the counts of profiles/walk_scalar_cost.log (131 scalar ALU
instructions, 60 branches; 155 and 69 before that change) plus a headroom of 6 and 3 for compiler drift."""
import collections
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tray_racing_amd", "csrc")
ASM = os.path.join(CSRC, "build", "kernels.s")

SALU_BOUND, BRANCH_BOUND = 131 + 6, 60 + 3

# scalar instructions that are not ALU work: branches (counted on their own), waits, no-ops, memory, messages
NOT_ALU = ("s_cbranch", "s_branch", "s_waitcnt", "s_nop", "s_load", "s_buffer_load", "s_barrier", "s_endpgm", "s_sleep",
           "s_setprio", "s_sendmsg", "s_trap", "s_icache", "s_setpc", "s_swappc", "s_getpc")


def headline_body(text):
    for m in re.finditer(r"\n(_ZN3trx\S*k_traceILi(\d)ELb(\d)ELi(\d)ELb(\d)ELb(\d)E\S*):", text):
        if tuple(int(x) for x in m.groups()[1:]) == (0, 0, 1, 0, 0):
            return text[m.end():text.index(".Lfunc_end", m.end())].splitlines()
    raise AssertionError("k_trace<0,false,1,false,false> not found")


def loops_of(body):
    """{loop header label: [depth, parent loop's header or None, instructions of the loop's own blocks]}, from the
    compiler's block comments ("in Loop: Header=BBn_m Depth=d", "Parent Loop BBn_m Depth=d", "This Loop Header: Depth=d")."""
    loops, cur, head, parents, in_comment = {}, None, None, [], False
    for line in body:
        s = line.strip()
        if re.match(r"^\.LBB\d+_\d+:|^; %bb\.\d+:", s):
            m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", s)
            cur = m.group(1) if m else None
            if cur:
                loops.setdefault(cur, [int(m.group(2)), None, []])
            label = re.match(r"^\.L(BB\d+_\d+):", s)
            head, parents, in_comment = (label.group(1) if label else None), [], True
            m = re.search(r"Parent Loop (BB\d+_\d+) Depth=", s)
            if m:
                parents.append(m.group(1))
            continue
        if in_comment and s.startswith(";"):
            m = re.search(r"Parent Loop (BB\d+_\d+) Depth=", s)
            if m:
                parents.append(m.group(1))
            m = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", s)
            if m and head:
                cur = head
                loops.setdefault(cur, [int(m.group(1)), None, []])
                loops[cur][1] = parents[-1] if parents else None
            continue
        if not s or s.startswith((";", ".")) or s.endswith(":"):
            continue
        in_comment = False
        if cur:
            loops[cur][2].append(s.split(";")[0].strip())
    return loops


def walk_loop_instructions(body):
    """The instructions of the largest depth-2 loop of the kernel - the plain walk's loop - with its child loops (the
    uniform step's per-child loop, the per-lane triangle rounds, the cooperative windows)."""
    loops = loops_of(body)
    depth2 = [h for h, v in loops.items() if v[0] == 2]
    assert depth2, "no depth-2 loop in the kernel"
    whole = {h: loops[h][2] + [i for k, v in loops.items() if v[1] == h for i in v[2]] for h in depth2}
    header = max(whole, key=lambda h: len(whole[h]))
    return whole[header], [k for k, v in loops.items() if v[1] == header]


def counts(instructions):
    c = collections.Counter()
    for i in instructions:
        op = i.split()[0]
        if op.startswith(("s_cbranch", "s_branch")):
            c["branch"] += 1
        elif op.startswith("s_") and not op.startswith(NOT_ALU):
            c["salu"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
    return c


@pytest.mark.skipif(not os.path.exists(ASM), reason="no device assembly (make -C tray_racing_amd/csrc build/kernels.s)")
def test_scalar_alu_and_branches_inside_the_walk_loop():
    instructions, children = walk_loop_instructions(headline_body(open(ASM).read()))
    c = counts(instructions)
    # (the loop found is the walk: its size and its three child loops)
    assert c["valu"] > 400 and len(children) == 3, (dict(c), children)
    assert c["salu"] <= SALU_BOUND, "scalar ALU instructions inside the walk loop: %d (bound %d)" % (c["salu"], SALU_BOUND)
    assert c["branch"] <= BRANCH_BOUND, "branches inside the walk loop: %d (bound %d)" % (c["branch"], BRANCH_BOUND)


def test_the_counter_on_a_hand_made_listing():
    """The parser on a listing small enough to count by hand: a depth-2 loop of two blocks with one child loop."""
    body = """
.LBB0_1:                                ; =>This Loop Header: Depth=1
	s_mov_b32 s0, 0
.LBB0_2:                                ;   Parent Loop BB0_1 Depth=1
                                        ; =>  This Loop Header: Depth=2
                                        ;       Child Loop BB0_3 Depth 3
	v_add_u32_e32 v0, v1, v2
	s_and_saveexec_b64 s[2:3], vcc
	s_cbranch_execz .LBB0_5
.LBB0_3:                                ;   Parent Loop BB0_1 Depth=1
                                        ;     Parent Loop BB0_2 Depth=2
                                        ; =>    This Inner Loop Header: Depth=3
	s_add_i32 s4, s4, -1
	s_cmp_lg_u32 s4, 0
	s_waitcnt lgkmcnt(0)
	s_cbranch_scc1 .LBB0_3
; %bb.4:                                ;   in Loop: Header=BB0_2 Depth=2
	s_nop 0
	v_mov_b32_e32 v3, 0
.LBB0_5:                                ;   in Loop: Header=BB0_2 Depth=2
	s_or_b64 exec, exec, s[2:3]
	s_cbranch_scc1 .LBB0_2
; %bb.6:                                ;   in Loop: Header=BB0_1 Depth=1
	s_branch .LBB0_1
""".splitlines()
    instructions, children = walk_loop_instructions(body)
    assert children == ["BB0_3"]
    assert dict(counts(instructions)) == {"valu": 2, "salu": 4, "branch": 3}
