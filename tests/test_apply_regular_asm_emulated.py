"""The apply routines of REGULAR centroid groups (apply_regular_asm_*, tools/gen_apply_asm.py
routine_regular()) and the routines the kernel calls, which hold them beside the general ones (apply_plan_asm_*, routine_plan()), under the interpreter of tools/emu_apply_asm.py: against the restated apply of tests/test_apply_asm_emulated.py and,
bit for bit, against the general routine of the same (ng, K, rotation, contract) on the same inputs.  A regular group is one whose
integer shifts grow by one per step; the routine takes the LDS position e0 = smax - shift[0] of the first step's b[j-1] and the step
count instead of a vector of shifts, and does per step without the general routine's tests.

Scalar ALU + branch instructions EXECUTED per group of n steps with regular shifts (interpreter counts, asserted below; the figures
DESIGN.md section 3.3 quotes):   general routine 2 + 9 n + (n - 1) // 2, regular routine 5 + 3 n + (n - 1) // 2 + n % 2 -- per step that
has a successor 9 against 3 (count-down, exit branch, offset add), every second one the loop's branch back in both, and an odd count's
last step jumps over the other last-step body.  n = 5: 49 against 23."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kiwi_amd", "csrc", "tools"))
import emu_apply_asm as emu  # noqa: E402
from tests.test_apply_asm_emulated import F32, reference, run_routine  # noqa: E402
from tests.test_apply_asm_emulated import ROUTINES as GENERAL  # noqa: E402

import gen_apply_asm as gen  # noqa: E402

CSRC = os.path.join(ROOT, "kiwi_amd", "csrc")
# the two families are generated text that is not committed (the build makes the plan family's file): straight from the generator
ROUTINES = dict(GENERAL)
for _fused in (False, True):
    for _ng in (10, 8):
        for _K in (5, 9):
            for _rot in (True, False):
                ROUTINES.update(emu.routines(gen.routine_regular(_ng, _K, _rot, _fused) + "\n" + gen.routine_plan(_ng, _K, _rot, _fused)))

SALU = ("s_mov_b32", "s_mov_b64", "s_add_u32", "s_addc_u32", "s_sub_i32", "s_sub_u32", "s_lshl_b32", "s_cmp_ge_u32", "s_cmp_lg_u32", "s_cmp_eq_u32")
BRANCH = ("s_branch", "s_cbranch_scc1")


def scalar_count(m):
    return sum(m.count.get(op, 0) for op in SALU + BRANCH)


def run_regular(name, lds, u0, e0, n, coef, cl, sl, acc, ins=None):
    m = emu.Machine(lds, coef)
    ar1, ar2, dz = acc
    # operands: %0 .. %5 = ar1a ar1b ar2a ar2b dza dzb, %6 abase, %7 e0, %8 n, %9 coef, %10 cl, %11 sl (emu.OPERANDS_REGULAR)
    for i, (A, c0) in enumerate(((ar1, 0), (ar1, 2), (ar2, 0), (ar2, 2), (dz, 0), (dz, 2))):
        m.v[200 + 2 * i] = A[:, c0].view(np.uint32)
        m.v[201 + 2 * i] = A[:, c0 + 1].view(np.uint32)
    m.v[212] = (4 * u0).astype(np.uint32)
    m.s[90], m.s[91] = e0, n
    m.s[92], m.s[93] = 0, 0
    m.s[94], m.s[95] = F32(cl).view(np.uint32), F32(sl).view(np.uint32)
    m.run(ROUTINES[name] if ins is None else ins, operands=emu.OPERANDS_REGULAR)
    out = []
    for i in range(3):
        out.append(np.stack([m.v[200 + 4 * i], m.v[201 + 4 * i], m.v[202 + 4 * i], m.v[203 + 4 * i]], 1).view(F32))
    return out, m


def run_plan(name, K, lds, u0, smax, shifts, e0, regular, coef, cl, sl, acc):
    """apply_plan_asm_*: the general routine's operands and the plan's header word (%13 = s96): flag bits, e0 in bits 4 .. 10, bit 11
    regular, the group length and the rest above (the routine must look at bits 4 .. 11 only)"""
    m = emu.Machine(lds, coef)
    ar1, ar2, dz = acc
    for i, (A, c0) in enumerate(((ar1, 0), (ar1, 2), (ar2, 0), (ar2, 2), (dz, 0), (dz, 2))):
        m.v[200 + 2 * i] = A[:, c0].view(np.uint32)
        m.v[201 + 2 * i] = A[:, c0 + 1].view(np.uint32)
    m.v[212] = (4 * u0).astype(np.uint32)
    ish = np.zeros(64, np.int64)
    if not regular:
        ish[:len(shifts)] = shifts                          # (a regular group's shifts are not loaded: the register holds zeros)
    m.v[213] = (ish & 0xffffffff).astype(np.uint32)
    m.s[90], m.s[91] = smax & 0xffffffff, len(shifts)
    m.s[92], m.s[93] = 0, 0
    m.s[94], m.s[95] = F32(cl).view(np.uint32), F32(sl).view(np.uint32)
    m.s[96] = 0x3 | ((e0 << 4) | (1 << 11) if regular else 0) | (len(shifts) << 16) | (1 << 23) | (37 << 24)
    m.run(ROUTINES[name], operands=emu.OPERANDS_PLAN)
    out = []
    for i in range(3):
        out.append(np.stack([m.v[200 + 4 * i], m.v[201 + 4 * i], m.v[202 + 4 * i], m.v[203 + 4 * i]], 1).view(F32))
    return out, m


def case(rng, K, n, e0_top, e0_cap=1 << 30):
    """shifts s0 + k; e0 = smax - s0 either 0 .. (with n - 1 below it the reads start at position e0 - (n - 1) >= 0: smax = s0 + n - 1,
    the smallest e0 a group of n can have) or the largest for which the last output's b[j] (position 63 + 192 + e0 + 1) is inside K * 64"""
    W = 10 * K * 64
    lds = rng.standard_normal(W).astype(F32)
    lds[rng.random(W) < 0.05] = 0.0
    u0 = np.arange(64)
    s0 = int(rng.integers(-5, 5))
    shifts = [s0 + k for k in range(n)]
    e0 = min((K * 64 - 1) - (63 + 192 + 1), e0_cap) if e0_top else n - 1
    assert e0 >= n - 1
    smax = s0 + e0
    coef = rng.standard_normal(20 * n).astype(F32)            # (exactly the group's lines: a load past the last step's is an error)
    cl, sl = F32(rng.standard_normal()), F32(rng.standard_normal())
    acc = [rng.standard_normal((64, 4)).astype(F32) for _ in range(3)]
    return lds, u0, smax, shifts, e0, coef, cl, sl, acc


@pytest.mark.parametrize("fused", [False, True], ids=["exact", "fused"])
@pytest.mark.parametrize("rot", [True, False], ids=["rot", "plain"])
@pytest.mark.parametrize("K", [5, 9])
@pytest.mark.parametrize("ng", [10, 8])
def test_regular_routine_equals_the_restated_apply_and_the_general_routine(ng, K, rot, fused):
    tail = "%d_k%d_%s_%s" % (ng, K, "rot" if rot else "plain", "fused" if fused else "exact")
    new, old = "apply_regular_asm_" + tail, "apply_group_asm_" + tail
    assert new in ROUTINES and old in ROUTINES
    rng = np.random.default_rng([20261019, K, int(rot), int(fused), ng])
    for e0_top in (False, True):
        for n in (1, 2, 3, 5, 8):
            lds, u0, smax, shifts, e0, coef, cl, sl, acc = case(rng, K, n, e0_top)
            if not e0_top and n == 1:
                assert e0 == 0
            want = reference(fused, rot, K, lds, u0, smax, shifts, coef, cl, sl, acc, ng)
            got, m = run_regular(new, lds, u0, e0, n, coef, cl, sl, acc)            # (a register read before its wait raises)
            gen, mo = run_routine(old, K, lds, u0, smax, shifts, coef, cl, sl, acc)
            for w, g, o, what in zip(want, got, gen, ("ar1", "ar2", "dz")):
                assert np.array_equal(w.view(np.uint32), g.view(np.uint32)), (new, n, e0, what)
                assert np.array_equal(o.view(np.uint32), g.view(np.uint32)), (new, old, n, e0, what)
            per_step = 4 * ng + (8 if rot else 0)
            if fused:
                assert m.count.get("v_pk_fma_f32", 0) + m.count.get("v_pk_mul_f32", 0) == per_step * n
            else:
                assert m.count["v_pk_mul_f32"] == per_step * n
            assert m.count.get("v_readlane_b32", 0) == 0
            assert scalar_count(m) < scalar_count(mo), (new, n, scalar_count(m), scalar_count(mo))
            # every step reads what the general routine reads, and the last one issues neither loads nor reads
            assert m.count["ds_read2st64_b32"] == mo.count["ds_read2st64_b32"] == 2 * ng * (n + 1)
            assert m.count.get("s_load_dwordx16", 0) == n
            assert scalar_count(m) == 5 + 3 * n + (n - 1) // 2 + n % 2
            assert scalar_count(mo) == 2 + 9 * n + (n - 1) // 2
            # instructions of every kind: seven fewer per step that has a successor, six per group (the shifts' way into the first address)
            assert sum(mo.count.values()) - sum(m.count.values()) == 6 + 7 * (n - 1) + (1 - n % 2)


@pytest.mark.parametrize("fused", [False, True], ids=["exact", "fused"])
@pytest.mark.parametrize("rot", [True, False], ids=["rot", "plain"])
@pytest.mark.parametrize("K", [5, 9])
@pytest.mark.parametrize("ng", [10, 8])
def test_plan_routine_takes_the_side_its_header_word_names(ng, K, rot, fused):
    """apply_plan_asm_* (what the kernel calls): with bit 11 of the header word set it executes the regular routine's instructions
    and three more (bit test, branch, the field's extraction; an even count's last step a fourth: the jump to the end), with the
    bit clear the general routine's and two more -- and gives their bits."""
    tail = "%d_k%d_%s_%s" % (ng, K, "rot" if rot else "plain", "fused" if fused else "exact")
    rng = np.random.default_rng([20261020, K, int(rot), int(fused), ng])
    for e0_top in (False, True):
        for n in (1, 2, 3, 5, 8):
            lds, u0, smax, shifts, e0, coef, cl, sl, acc = case(rng, K, n, e0_top, e0_cap=0x7f)      # (the header word's field: seven bits)
            want = reference(fused, rot, K, lds, u0, smax, shifts, coef, cl, sl, acc, ng)
            _, mr = run_regular("apply_regular_asm_" + tail, lds, u0, e0, n, coef, cl, sl, acc)
            _, mg = run_routine("apply_group_asm_" + tail, K, lds, u0, smax, shifts, coef, cl, sl, acc)
            for regular, other in ((True, mr), (False, mg)):
                got, m = run_plan("apply_plan_asm_" + tail, K, lds, u0, smax, shifts, e0, regular, coef, cl, sl, acc)
                for w, g, what in zip(want, got, ("ar1", "ar2", "dz")):
                    assert np.array_equal(w.view(np.uint32), g.view(np.uint32)), (tail, regular, n, e0, what)
                extra = (3 + (1 - n % 2)) if regular else 2
                assert sum(m.count.values()) == sum(other.count.values()) + extra
                assert m.count.get("v_readlane_b32", 0) == (0 if regular else other.count["v_readlane_b32"])
                assert m.count["ds_read2st64_b32"] == other.count["ds_read2st64_b32"]


def test_generator_prints_each_family_as_a_file_of_its_own():
    """`gen_apply_asm.py regular|plan` print the sixteen routines of the family per contract block, under a megabyte; without an argument
    the general family as before (tests/test_generated_sources.py)"""
    import subprocess
    env = dict(os.environ)
    env.pop("KIWI_ASM_VARIANT", None)
    for family in ("regular", "plan"):
        out = subprocess.run([sys.executable, os.path.join(CSRC, "tools", "gen_apply_asm.py"), family], capture_output=True, text=True, env=env, check=True).stdout
        got = emu.routines(out)
        assert len(got) == 16 and all(k.startswith("apply_%s_asm_" % family) and ROUTINES[k] == v for k, v in got.items())
        assert out.count("#if KIWI_ARITH == ") == 2 and len(out) < (1 << 20)


def test_regular_routine_without_its_wait_is_refused():
    name = "apply_regular_asm_10_k5_rot_exact"
    broken = [i for i in ROUTINES[name] if not i.startswith("s_waitcnt")]
    rng = np.random.default_rng(11)
    lds, u0, smax, shifts, e0, coef, cl, sl, acc = case(rng, 5, 3, False)
    with pytest.raises(emu.EmuError):
        run_regular(name, lds, u0, e0, 3, coef, cl, sl, acc, ins=broken)
