"""The routines accumulate_multi_kernel calls where it has plans (apply_steps_asm_*, tools/gen_apply_asm.py routine_steps()) under the
interpreter of tools/emu_apply_asm.py.  One statement, a three-way choice on the plan's header word (PlanSrc::head): bit 11 -- the
regular text; a bit of 12 .. 15 -- the text for groups of at most five steps whose shifts grow by one or STAY (bit 12 + j: step j + 1 has
step j's shift), lines_repeat(); neither -- the general text.

A step whose successor stays reads nothing: the successor's b[j] and b[j-1] are the two banks as they stand.  So a group of n steps with
u successors one sample on issues 2 NG (2 + u) tile reads -- both banks once, one bank per "+1" -- where the general routine issues
2 NG (2 + u + 2 (n - 1 - u)), and the n coefficient lines once each; the successor's line, loaded into the other buffer, is copied into
the buffer at hand behind a wait, which the interpreter's "register read before its wait" check watches.  Results: the restated apply of
tests/test_apply_asm_emulated.py and the general routine of the same (ng, K, rotation, contract), bit for bit."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kiwi_amd", "csrc", "tools"))
import emu_apply_asm as emu  # noqa: E402
from tests.test_apply_asm_emulated import F32, reference, run_routine  # noqa: E402
from tests.test_apply_asm_emulated import ROUTINES as GENERAL  # noqa: E402
from tests.test_apply_regular_asm_emulated import case, run_regular  # noqa: E402
from tests.test_apply_regular_asm_emulated import ROUTINES as REGULAR  # noqa: E402

import gen_apply_asm as gen  # noqa: E402

CSRC = os.path.join(ROOT, "kiwi_amd", "csrc")
COMBOS = [(ng, K, rot, fused) for fused in (False, True) for ng in (10, 8) for K in (5, 9) for rot in (True, False)]
ROUTINES = {}
for _c in COMBOS:
    ROUTINES.update(emu.routines(gen.routine_steps(*_c)))
ONE_TEXT = {}
for _c in COMBOS:
    ONE_TEXT.update(emu.routines(gen.routine_steps(*_c, one_text=True)))


def tail_of(ng, K, rot, fused):
    return "%d_k%d_%s_%s" % (ng, K, "rot" if rot else "plain", "fused" if fused else "exact")


def run_steps(ins, lds, u0, smax, shifts, head_bits, load_shifts, coef, cl, sl, acc):
    """apply_steps_asm_*: the general routine's operands and the plan's header word (%13 = s96): flag bits, head_bits (e0, bit 11, the
    mask), the group length and the rest above (the routine must look at bits 4 .. 15 only)"""
    m = emu.Machine(lds, coef)
    ar1, ar2, dz = acc
    for i, (A, c0) in enumerate(((ar1, 0), (ar1, 2), (ar2, 0), (ar2, 2), (dz, 0), (dz, 2))):
        m.v[200 + 2 * i] = A[:, c0].view(np.uint32)
        m.v[201 + 2 * i] = A[:, c0 + 1].view(np.uint32)
    m.v[212] = (4 * u0).astype(np.uint32)
    ish = np.zeros(64, np.int64)
    if load_shifts:
        ish[:len(shifts)] = shifts                          # (the kernel loads the shifts of a general group only)
    m.v[213] = (ish & 0xffffffff).astype(np.uint32)
    m.s[90], m.s[91] = smax & 0xffffffff, len(shifts)
    m.s[92], m.s[93] = 0, 0
    m.s[94], m.s[95] = F32(cl).view(np.uint32), F32(sl).view(np.uint32)
    m.s[96] = 0x3 | head_bits | (len(shifts) << 16) | (1 << 23) | (37 << 24)
    m.run(ins, operands=emu.OPERANDS_PLAN)
    out = []
    for i in range(3):
        out.append(np.stack([m.v[200 + 4 * i], m.v[201 + 4 * i], m.v[202 + 4 * i], m.v[203 + 4 * i]], 1).view(F32))
    return out, m


def masked_case(rng, K, n, mask, end):
    """case()'s tile, coefficients and accumulators with the shifts of `mask` (bit j: step j + 1 stays) and e0 = smax - shifts[0] at
    case()'s small end (n - 1), at the group's own smallest (the number of its "+1" successors: the last step's b[j-1] is position 0)
    or at the largest the header word and the tile allow"""
    lds, u0, smax, shifts, e0, coef, cl, sl, acc = case(rng, K, n, end == "top", e0_cap=0x7f)
    s = [shifts[0]]
    for j in range(n - 1):
        s.append(s[-1] + (0 if (mask >> j) & 1 else 1))
    ups = s[-1] - s[0]
    if end == "least":
        e0 = ups
        smax = s[0] + e0
    assert ups <= e0 <= 0x7f and smax - s[0] == e0
    return lds, u0, smax, s, e0, ups, coef, cl, sl, acc


def same(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def every_mask(ins, ng, K, rot, fused):
    tail = tail_of(ng, K, rot, fused)
    rng = np.random.default_rng([20261101, K, int(rot), int(fused), ng])
    per_step = 4 * ng + (8 if rot else 0)
    for n in (2, 3, 4, 5):
        for mask in range(1, 1 << (n - 1)):
            for end in ("small", "least", "top"):
                lds, u0, smax, shifts, e0, ups, coef, cl, sl, acc = masked_case(rng, K, n, mask, end)
                want = reference(fused, rot, K, lds, u0, smax, shifts, coef, cl, sl, acc, ng)
                old, mo = run_routine("apply_group_asm_" + tail, K, lds, u0, smax, shifts, coef, cl, sl, acc)
                got, m = run_steps(ins, lds, u0, smax, shifts, (e0 << 4) | (mask << 12), False, coef, cl, sl, acc)   # (a register read before its wait raises)
                assert same(want, got), (tail, n, mask, e0)
                assert same(old, got), (tail, n, mask, e0)
                assert m.count["ds_read2st64_b32"] == 2 * ng * (2 + ups)
                assert mo.count["ds_read2st64_b32"] == 2 * ng * (2 + ups + 2 * (n - 1 - ups))
                assert m.count["s_load_dwordx16"] == n
                assert m.count.get("s_load_dwordx4", 0) == (n if ng == 10 else 0)
                assert m.count.get("v_readlane_b32", 0) == 0
                assert m.count.get("s_mov_b64", 0) == 1 + ng * (n - 1 - ups)      # (the coefficient pointer; a line per step that stays)
                muls = m.count.get("v_pk_mul_f32", 0) + (m.count.get("v_pk_fma_f32", 0) if fused else 0)
                assert muls == per_step * n
                assert sum(m.count.values()) < sum(mo.count.values())


@pytest.mark.parametrize("fused", [False, True], ids=["exact", "fused"])
@pytest.mark.parametrize("rot", [True, False], ids=["rot", "plain"])
@pytest.mark.parametrize("K", [5, 9])
@pytest.mark.parametrize("ng", [10, 8])
def test_every_mask_of_two_to_five_steps(ng, K, rot, fused):
    every_mask(ROUTINES["apply_steps_asm_" + tail_of(ng, K, rot, fused)], ng, K, rot, fused)


@pytest.mark.parametrize("ng,K,rot,fused", [(10, 5, True, False), (8, 9, False, True)])
def test_every_mask_with_the_one_text_variant(ng, K, rot, fused):
    """the A/B variant of the generator (`steps-one-text`: regular groups take the text of the masked ones too) on two of the sixteen"""
    every_mask(ONE_TEXT["apply_steps_asm_" + tail_of(ng, K, rot, fused)], ng, K, rot, fused)


@pytest.mark.parametrize("fused", [False, True], ids=["exact", "fused"])
@pytest.mark.parametrize("rot", [True, False], ids=["rot", "plain"])
@pytest.mark.parametrize("K", [5, 9])
@pytest.mark.parametrize("ng", [10, 8])
def test_the_other_two_sides_are_the_regular_and_the_general_text(ng, K, rot, fused):
    """bit 11: apply_regular_asm_*'s instructions and three more (bit test, branch, the field's extraction; an even count's last step a
    fourth: the jump to the end), as in apply_plan_asm_*.  Neither bit 11 nor a mask: the general routine's and four more (two tests,
    two branches).  Their bits in both."""
    tail = tail_of(ng, K, rot, fused)
    rng = np.random.default_rng([20261102, K, int(rot), int(fused), ng])
    for e0_top in (False, True):
        for n in (1, 2, 3, 5, 8):
            lds, u0, smax, shifts, e0, coef, cl, sl, acc = case(rng, K, n, e0_top, e0_cap=0x7f)
            want = reference(fused, rot, K, lds, u0, smax, shifts, coef, cl, sl, acc, ng)
            _, mr = run_regular("apply_regular_asm_" + tail, lds, u0, e0, n, coef, cl, sl, acc)
            _, mg = run_routine("apply_group_asm_" + tail, K, lds, u0, smax, shifts, coef, cl, sl, acc)
            for regular, other in ((True, mr), (False, mg)):
                got, m = run_steps(ROUTINES["apply_steps_asm_" + tail], lds, u0, smax, shifts, ((e0 << 4) | (1 << 11)) if regular else 0,
                                   not regular, coef, cl, sl, acc)
                assert same(want, got), (tail, regular, n, e0)
                extra = (3 + (1 - n % 2)) if regular else 4
                assert sum(m.count.values()) == sum(other.count.values()) + extra
                for op in ("ds_read2st64_b32", "v_readlane_b32", "s_load_dwordx16", "v_pk_mul_f32", "v_pk_add_f32", "v_pk_fma_f32", "s_waitcnt"):
                    assert m.count.get(op, 0) == other.count.get(op, 0), op
            # (the one-text variant: a regular group of any length takes the text of the masked ones, the general side is the same)
            got, m = run_steps(ONE_TEXT["apply_steps_asm_" + tail], lds, u0, smax, shifts, (e0 << 4) | (1 << 11), False, coef, cl, sl, acc)
            assert same(want, got) and m.count["ds_read2st64_b32"] == mr.count["ds_read2st64_b32"] and m.count.get("v_readlane_b32", 0) == 0
            got, m = run_steps(ONE_TEXT["apply_steps_asm_" + tail], lds, u0, smax, shifts, 0, True, coef, cl, sl, acc)
            assert same(want, got) and sum(m.count.values()) == sum(mg.count.values()) + 2


def test_the_text_of_the_old_sides_is_unchanged():
    """the regular and the general side of the statement are lines_regular()'s and lines_general()'s, instruction for instruction"""
    for c in COMBOS:
        tail = tail_of(*c)
        ins = ROUTINES["apply_steps_asm_" + tail]
        plan = REGULAR["apply_plan_asm_" + tail]
        cut = plan.index(".Lkiwi_general_:")
        at = ins.index(".Lkiwi_notregular_:")
        assert ins[2:at] == plan[2:cut]
        assert ins[ins.index(".Lkiwi_general_:"):] == plan[cut:] == [".Lkiwi_general_:"] + GENERAL["apply_group_asm_" + tail]


def test_generator_prints_the_family_as_a_file_of_its_own():
    import subprocess
    env = dict(os.environ)
    env.pop("KIWI_ASM_VARIANT", None)
    for family, want in (("steps", ROUTINES), ("steps-one-text", ONE_TEXT)):
        out = subprocess.run([sys.executable, os.path.join(CSRC, "tools", "gen_apply_asm.py"), family], capture_output=True, text=True, env=env, check=True).stdout
        got = emu.routines(out)
        assert len(got) == 16 and got == want
        assert out.count("#if KIWI_ARITH == ") == 2


def test_copy_of_the_coefficient_line_without_its_wait_is_refused():
    """the wait in front of the copy is the only thing between the successor's line being loaded and being read"""
    name = "apply_steps_asm_10_k5_rot_exact"
    ins = list(ROUTINES[name])
    at = ins.index(".Lkiwi_prep0_:")
    w = at + 1 + ins[at + 1:].index("s_waitcnt lgkmcnt(0)")
    assert ins[w + 1].startswith("s_mov_b64")
    broken = ins[:w] + ins[w + 1:]
    rng = np.random.default_rng(12)
    lds, u0, smax, shifts, e0, ups, coef, cl, sl, acc = masked_case(rng, 5, 3, 0b01, "small")
    run_steps(ins, lds, u0, smax, shifts, (e0 << 4) | (0b01 << 12), False, coef, cl, sl, acc)
    with pytest.raises(emu.EmuError):
        run_steps(broken, lds, u0, smax, shifts, (e0 << 4) | (0b01 << 12), False, coef, cl, sl, acc)
