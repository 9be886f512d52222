#!/usr/bin/env python3
"""Generates kiwi_apply_asm.inc: the apply of ONE centroid group of accumulate_multi_kernel as a single hand-allocated
assembly routine (round 4).  python tools/gen_apply_asm.py > kiwi_apply_asm.inc

Why assembly: the apply wants the LDS reads of step k + 1 in flight while the arithmetic of step k runs, plus the next step's
coefficient line in a second scalar buffer.  With the shift moving by one sample per step (the regular case) step k + 1 needs only
its b[j-1] -- its b[j] is step k's b[j-1], in place --, and a register pair of step k's b[j] set is free the moment its one multiply
has issued: the next step's b[j-1] is read INTO it right there ("read behind").  Two register sets that swap roles every step, every
read of a step issued 100-400 cycles before the step needs it.  Written in C++ with asm read statements (three sets; the compiler
cannot express the read-behind) the register allocator needs 244 vector registers ("What did not pay in round
4" (iii)); allocated by hand it is 80 + 20.  The routine fixes its registers (clobber lists) and takes the accumulators, the LDS
address, the shifts and the coefficient pointer as operands.

Per accumulator the operations and their order are carry2_apply's (the reference's): application order of the GF components
1 2 3 [9] -> radial sum t1, 4 5 -> transverse sum t2, 6 7 8 [10] -> vertical; per component  T += wl * b[j];  T += wr * b[j-1]
(sparse_trace.f90:684-703), then the rotation by the back-azimuth change (seismogram.f90:196-203).  Radial and vertical
components are issued alternately (independent accumulators: four dependency chains instead of two).
exact: v_pk_mul_f32 + v_pk_add_f32, every product and sum rounded on its own.   fused: v_pk_fma_f32.

Registers (kernel budget: 168 VGPRs at three waves per SIMD):
  v[28:35]  t1a t1b t2a t2b     v[36:43] m0..m3 (products, exact only)     v44 va  v45 va4  v46 vn  v47 vn4
  v[48:87] bank 0   v[88:127] bank 1      (member m of a bank: pair 2m; m < NG: outputs q0,q1 of the m-th component in application
                                          order, m >= NG: outputs q2,q3)
  s[36:55], s[56:75] coefficient lines of the step at hand and of the next one, swapping roles every step   s[76:77] (cl, sl)
  s80 k  s81, s82 4 x integer shift of this step / the next (swapping)  s83 tmp  s84 4 d  s[86:87] coefficient pointer
  v44 address of position smax  v45 4 x shifts (lane k: step k)  v46, v47 addresses of the next reads

Three more families (python tools/gen_apply_asm.py regular | plan | steps; not committed: the Makefile writes the steps family into
build/kiwi_apply_steps_asm.inc, the tests call the generator): apply_regular_asm_* serves the groups whose shifts grow by one per step
(routine_regular()); apply_plan_asm_* holds that text and the general routine's in one statement (routine_plan(): what
accumulate_multi_kernel called where it has plans until the plans named repeated shifts; kept as it is, tests/
test_apply_regular_asm_emulated.py pins its instruction counts); apply_steps_asm_*, what the kernel calls there now, holds a third text
beside the two, for groups of at most five steps whose shifts grow by one or stay (lines_repeat(), routine_steps()): a step whose
successor has its shift reads no tile -- both banks are the successor's as they stand -- and copies the successor's coefficient line into
the buffer at hand, so that banks and buffers keep their parity and the same step text runs again.  s84: the plan's repeat bits, s82:
number of the successor's bit.  `steps-one-text` prints the A/B variant in which regular groups take that third text too.
"""
import os
import sys

VARIANT = set(filter(None, os.environ.get('KIWI_ASM_VARIANT', '').split(',')))     # timing experiments only (wrong results)

SEQ = {10: [0, 1, 2, 8, 3, 4, 5, 6, 7, 9], 8: [0, 1, 2, 3, 4, 5, 6, 7]}
BANK = [48, 88]
T1A, T1B, T2A, T2B = 28, 30, 32, 34
M = [36, 38, 40, 42]
VA, VA4, VN, VN4 = 44, 45, 46, 47
CA, CB, CLSL = 36, 56, 76
SK, SE, SEN, ST, SD, SK1, SCP = 80, 81, 82, 83, 84, 85, 86


def vp(r):
    return "v[%d:%d]" % (r, r + 1)


def sp(r):
    return "s[%d:%d]" % (r, r + 1)


def member(bank, m):
    return BANK[bank] + 2 * m


def reads(bank, ng, K, addr):
    out = []
    for m in range(2 * ng):
        o = SEQ[ng][m % ng] * K + (2 if m >= ng else 0)
        out.append("ds_read2st64_b32 %s, v%d offset0:%d offset1:%d" % (vp(member(bank, m)), addr, o, o + 1))
    return out


def mac(fused, T, cpair, hi, X, tmp, first=False):
    """T += c * X  (c = low / high half of the scalar pair), as one or two instructions; first: T = 0 + c * X"""
    sel = "op_sel:[1,0]" if hi else "op_sel_hi:[0,1]"
    if fused and not first:
        sel3 = "op_sel:[1,0,0]" if hi else "op_sel_hi:[0,1,1]"
        return ["v_pk_fma_f32 %s, %s, %s, %s %s" % (vp(T), sp(cpair), vp(X), vp(T), sel3)], []
    mul = "v_pk_mul_f32 %s, %s, %s %s" % (vp(tmp), sp(cpair), vp(X), sel)
    if first:
        add = "v_pk_add_f32 %s, %s, 0 op_sel_hi:[1,0]" % (vp(T), vp(tmp))
    else:
        add = "v_pk_add_f32 %s, %s, %s" % (vp(T), vp(T), vp(tmp))
    return [mul], [add]


def arithmetic(ng, rot, fused, H, L, acc, K=None, behind=False, C=None):
    """instruction list of one step: acc = operand names of ar1a ar1b ar2a ar2b dza dzb.  behind: behind the multiplies that
    consume a member of the b[j] bank H, the NEXT step's b[j-1] of that member is read into its registers (address VN)"""
    nH1 = 4 if ng == 10 else 3
    nH = nH1 + 2
    ar1a, ar1b, ar2a, ar2b, dza, dzb = acc
    out = []
    t1 = (T1A, T1B) if rot else None
    t2 = (T2A, T2B) if rot else None

    def tgt(a):
        if a < nH1:
            return (vp(T1A), vp(T1B)) if rot else (ar1a, ar1b)
        if a < nH:
            return (vp(T2A), vp(T2B)) if rot else (ar2a, ar2b)
        return (dza, dzb)

    def emit_pair(items):
        """items: list of (a) application indices issued together (independent accumulators); each contributes
        Ta += wl*H.a; Tb += wl*H.b; Ta += wr*L.a; Tb += wr*L.b"""
        for half, src in ((False, H), (True, L)):          # wl * b[j] first, then wr * b[j-1]
            muls, adds = [], []
            ti = 0
            for a in items:
                Ta, Tb = tgt(a)
                cpair = C + 2 * a
                first = rot and (not half) and (a == 0 or a == nH1)      # t1 / t2 start from 0 + product
                for T, m in ((Ta, a), (Tb, ng + a)):
                    X = member(src, m)
                    tmp = M[ti % 4]
                    ti += 1
                    sel = "op_sel:[1,0]" if half else "op_sel_hi:[0,1]"
                    if first:
                        # t = 0 + p (the reference zeroes the sum, then adds) differs from t = p only where p is -0, and a
                        # sum that differs in the sign of a zero never reaches an output bit: t1 / t2 are only multiplied by
                        # cl / sl and ADDED to accumulators that start from +0 -- a round-to-nearest sum is -0 only if both
                        # operands are, so those are never -0, and x + (+-0) = x for every other x (NaN, infinities alike)
                        muls.append("v_pk_mul_f32 %s, %s, %s %s" % (T, sp(cpair), vp(X), sel))
                    elif fused:
                        sel3 = "op_sel:[1,0,0]" if half else "op_sel_hi:[0,1,1]"
                        muls.append("v_pk_fma_f32 %s, %s, %s, %s %s" % (T, sp(cpair), vp(X), T, sel3))
                    else:
                        muls.append("v_pk_mul_f32 %s, %s, %s %s" % (vp(tmp), sp(cpair), vp(X), sel))
                        adds.append("v_pk_add_f32 %s, %s, %s" % (T, T, vp(tmp)))
            out.extend(muls)
            if behind and not half:
                for a in items:
                    for m in (a, ng + a):
                        o = SEQ[ng][m % ng] * K + (2 if m >= ng else 0)
                        out.append("ds_read2st64_b32 %s, v%d offset0:%d offset1:%d" % (vp(member(H, m)), VN, o, o + 1))
            out.extend(adds)

    # radial and vertical components alternately, then the transverse pair, then the rotation
    for i in range(nH1):
        emit_pair([i, nH + i])
    emit_pair([nH1])
    emit_pair([nH1 + 1])
    if rot:
        # ar1 = ar1 + cl*t1 - sl*t2 ; ar2 = ar2 + cl*t2 + sl*t1   (seismogram.f90:200-203), cl = s76, sl = s77
        cl, sl = "op_sel_hi:[0,1]", "op_sel:[1,0]"
        if fused:
            cl3, sl3 = "op_sel_hi:[0,1,1]", "op_sel:[1,0,0]"
            out += ["v_pk_fma_f32 %s, %s, %s, %s %s" % (ar1a, sp(CLSL), vp(T1A), ar1a, cl3),
                    "v_pk_fma_f32 %s, %s, %s, %s %s" % (ar1b, sp(CLSL), vp(T1B), ar1b, cl3),
                    "v_pk_fma_f32 %s, %s, %s, %s %s" % (ar2a, sp(CLSL), vp(T2A), ar2a, cl3),
                    "v_pk_fma_f32 %s, %s, %s, %s %s" % (ar2b, sp(CLSL), vp(T2B), ar2b, cl3),
                    "v_pk_fma_f32 %s, %s, %s, %s %s neg_lo:[0,1,0] neg_hi:[0,1,0]" % (ar1a, sp(CLSL), vp(T2A), ar1a, sl3),
                    "v_pk_fma_f32 %s, %s, %s, %s %s neg_lo:[0,1,0] neg_hi:[0,1,0]" % (ar1b, sp(CLSL), vp(T2B), ar1b, sl3),
                    "v_pk_fma_f32 %s, %s, %s, %s %s" % (ar2a, sp(CLSL), vp(T1A), ar2a, sl3),
                    "v_pk_fma_f32 %s, %s, %s, %s %s" % (ar2b, sp(CLSL), vp(T1B), ar2b, sl3)]
        else:
            out += ["v_pk_mul_f32 %s, %s, %s %s" % (vp(M[0]), sp(CLSL), vp(T1A), cl),
                    "v_pk_mul_f32 %s, %s, %s %s" % (vp(M[1]), sp(CLSL), vp(T1B), cl),
                    "v_pk_mul_f32 %s, %s, %s %s" % (vp(M[2]), sp(CLSL), vp(T2A), cl),
                    "v_pk_mul_f32 %s, %s, %s %s" % (vp(M[3]), sp(CLSL), vp(T2B), cl),
                    "v_pk_add_f32 %s, %s, %s" % (ar1a, ar1a, vp(M[0])),
                    "v_pk_add_f32 %s, %s, %s" % (ar1b, ar1b, vp(M[1])),
                    "v_pk_add_f32 %s, %s, %s" % (ar2a, ar2a, vp(M[2])),
                    "v_pk_add_f32 %s, %s, %s" % (ar2b, ar2b, vp(M[3])),
                    "v_pk_mul_f32 %s, %s, %s %s" % (vp(M[0]), sp(CLSL), vp(T2A), sl),
                    "v_pk_mul_f32 %s, %s, %s %s" % (vp(M[1]), sp(CLSL), vp(T2B), sl),
                    "v_pk_mul_f32 %s, %s, %s %s" % (vp(M[2]), sp(CLSL), vp(T1A), sl),
                    "v_pk_mul_f32 %s, %s, %s %s" % (vp(M[3]), sp(CLSL), vp(T1B), sl),
                    "v_pk_add_f32 %s, %s, %s neg_lo:[0,1] neg_hi:[0,1]" % (ar1a, ar1a, vp(M[0])),
                    "v_pk_add_f32 %s, %s, %s neg_lo:[0,1] neg_hi:[0,1]" % (ar1b, ar1b, vp(M[1])),
                    "v_pk_add_f32 %s, %s, %s" % (ar2a, ar2a, vp(M[2])),
                    "v_pk_add_f32 %s, %s, %s" % (ar2b, ar2b, vp(M[3]))]
    return out


def routine(ng, K, rot, fused):
    name = "apply_group_asm_%d_k%d_%s_%s" % (ng, K, "rot" if rot else "plain", "fused" if fused else "exact")
    return wrap_general(name, lines_general(ng, K, rot, fused))


def lines_general(ng, K, rot, fused):
    acc = ["%0", "%1", "%2", "%3", "%4", "%5"]
    # operands: %6 abase (v), %7 ishv (v), %8 smax (s), %9 n (s), %10 coef (s, 64 bit), %11 cl (s), %12 sl (s)
    L = []
    a = L.append
    SI = [SE, SEN]                        # 4 x integer shift of the step at hand / of the next one, swapping roles like the register sets
    a("s_mov_b32 s%d, %%11" % CLSL)
    a("s_mov_b32 s%d, %%12" % (CLSL + 1))
    a("s_mov_b64 %s, %%10" % sp(SCP))
    a("s_mov_b32 s%d, 0" % SK)
    a("s_load_dwordx16 s[%d:%d], %s, 0x0" % (CA, CA + 15, sp(SCP)))
    if ng == 10:
        a("s_load_dwordx4 s[%d:%d], %s, 0x40" % (CA + 16, CA + 19, sp(SCP)))
    a("v_lshlrev_b32 v%d, 2, %%7" % VA4)               # v45: 4 x the steps' integer shifts (lane k: step k)
    a("s_lshl_b32 s%d, %%8, 2" % ST)
    a("v_add_u32 v%d, s%d, %%6" % (VA, ST))           # v44: LDS address of position smax of the lane's first sample ...
    a("s_nop 1")                                       # (a vector register written by the instruction in front is not yet there for v_readlane)
    a("v_readlane_b32 s%d, v%d, 0" % (SI[0], VA4))
    a("v_subrev_u32 v%d, s%d, v%d" % (VN, SI[0], VA))  # ... of position e = smax - ishift: b[j-1] of step 0
    a("v_add_u32 v%d, 4, v%d" % (VN4, VN))
    L += reads(0, ng, K, VN4)            # bank 0 = b[j]
    L += reads(1, ng, K, VN)             # bank 1 = b[j-1]
    tail = []                            # the steps without a regular successor: out of line, the regular path falls through
    for r in range(2):
        H, Lb = r, 1 - r
        Cc, Cn = (CA, CB) if r == 0 else (CB, CA)        # the two coefficient buffers swap roles with the register sets
        a(".Lkiwi_step%d_%%=:" % r)
        a("s_waitcnt lgkmcnt(0)")
        a("s_add_u32 s%d, s%d, 1" % (SK, SK))
        a("s_mov_b32 s%d, 0x7fffffff" % SD)      # d = 0x7fffffff: "no successor" (neither read-behind nor reads behind the step)
        a("s_cmp_ge_u32 s%d, %%9" % SK)
        a("s_cbranch_scc1 .Lkiwi_plain%d_%%=" % r)
        a("v_readlane_b32 s%d, v%d, s%d" % (SI[1 - r], VA4, SK))
        a("s_add_u32 s%d, s%d, %d" % (SCP, SCP, 80))
        a("s_addc_u32 s%d, s%d, 0" % (SCP + 1, SCP + 1))
        a("s_load_dwordx16 s[%d:%d], %s, 0x0" % (Cn, Cn + 15, sp(SCP)))
        if ng == 10:
            a("s_load_dwordx4 s[%d:%d], %s, 0x40" % (Cn + 16, Cn + 19, sp(SCP)))
        a("s_sub_i32 s%d, s%d, s%d" % (SD, SI[1 - r], SI[r]))     # 4 x (positions the tile moves back by)
        a("v_subrev_u32 v%d, s%d, v%d" % (VN, SI[1 - r], VA))
        a("s_cmp_lg_u32 s%d, 4" % SD)
        a("s_cbranch_scc1 .Lkiwi_plain%d_%%=" % r)
        # regular successor: its b[j-1] is read behind this step's multiplies, into the b[j] bank
        L += arithmetic(ng, rot, fused, H, Lb, acc, K, True, C=Cc)
        if r == 1:
            a("s_branch .Lkiwi_step0_%=")
        t = tail.append
        t(".Lkiwi_plain%d_%%=:" % r)
        tail += arithmetic(ng, rot, fused, H, Lb, acc, C=Cc)
        t("s_cmp_eq_u32 s%d, 0x7fffffff" % SD)
        t("s_cbranch_scc1 .Lkiwi_end_%=")
        # irregular successor: its b[j] over this step's b[j-1] bank, its b[j-1] over the b[j] bank
        t("v_add_u32 v%d, 4, v%d" % (VN4, VN))
        tail += reads(Lb, ng, K, VN4)
        tail += reads(H, ng, K, VN)
        t("s_branch .Lkiwi_step%d_%%=" % (1 - r))
    L += tail
    a(".Lkiwi_end_%=:")
    if VARIANT:
        steps = [i for i, x in enumerate(L) if x.startswith(".Lkiwi_step0")][0]
        def keep(i, x):
            if "noarith" in VARIANT and x.startswith("v_pk_"): return False
            if "nolds" in VARIANT and i > steps and x.startswith("ds_read"): return False
            if "nocoef" in VARIANT and i > steps and x.startswith("s_load"): return False
            return True
        L = [x for i, x in enumerate(L) if keep(i, x)]
    return L


def wrap_general(name, L, head=False):
    """the routine's C++ function: routine()'s operands, and behind them (head) the plan's header word in a scalar register"""
    text = "\\n\\t\"\n        \"".join(L)
    clob_v = ", ".join('"v%d"' % i for i in range(28, 128))
    clob_s = ", ".join('"s%d"' % i for i in list(range(CA, CB + 20)) + [CLSL, CLSL + 1] + list(range(SK, SCP + 2)))
    out = []
    out.append("__device__ __forceinline__ void %s(f2v &ar1a, f2v &ar1b, f2v &ar2a, f2v &ar2b, f2v &dza, f2v &dzb, unsigned abase, int ishv,\n"
               "        int smax, int n, const float *coef, float cl, float sl%s)" % (name, ", int head" if head else ""))
    out.append("{")
    out.append('    asm volatile(\n        "%s\\n\\t"' % text)
    out.append('        : "+v"(ar1a), "+v"(ar1b), "+v"(ar2a), "+v"(ar2b), "+v"(dza), "+v"(dzb)')
    out.append('        : "v"(abase), "v"(ishv), "s"(smax), "s"(n), "s"(coef), "s"(cl), "s"(sl)%s' % (', "s"(head)' if head else ""))
    out.append('        : "memory", "scc", "vcc", %s,\n          %s);' % (clob_s, clob_v))
    out.append("}")
    return "\n".join(out)


def routine_regular(ng, K, rot, fused):
    """The apply of a REGULAR group: every centroid's integer shift is its predecessor's + 1 (multi_plan_kernel decides it once per
    evaluation, PlanSrc::head).  What routine() establishes again at every step -- the next shift out of a vector register, its
    difference to this one's, whether that is one sample -- is known, so the step's bookkeeping is a count-down whose borrow is the
    exit branch, one add on the coefficient offset (the scalar loads take it from a register: no 64-bit pointer add) and one add on
    the read address.  The step bodies are arithmetic()'s, the ones routine() takes for a regular successor and for a last step:
    per accumulator the same operations in the same order.
    Registers as routine()'s, except: s80 steps left behind this one, s85 byte offset of the next coefficient line, no v44 / v45 and
    no s81 / s82 / s84."""
    name = "apply_regular_asm_%d_k%d_%s_%s" % (ng, K, "rot" if rot else "plain", "fused" if fused else "exact")
    # operands: %6 abase (v), %7 e0 (s), %8 n (s), %9 coef (s, 64 bit), %10 cl (s), %11 sl (s)
    L = lines_regular(ng, K, rot, fused, {"abase": "%6", "e0": "%7", "n": "%8", "coef": "%9", "cl": "%10", "sl": "%11"}, ".Lkiwi_rend_%=", False)
    L.append(".Lkiwi_rend_%=:")
    return wrap_regular(name, L)


def prologue_regular(ng, K, op):
    """what lines_regular() and lines_repeat() do in front of their steps: rotation, the first coefficient line, the counters, both banks"""
    L = []
    a = L.append
    a("s_mov_b32 s%d, %s" % (CLSL, op["cl"]))
    a("s_mov_b32 s%d, %s" % (CLSL + 1, op["sl"]))
    a("s_mov_b64 %s, %s" % (sp(SCP), op["coef"]))
    a("s_load_dwordx16 s[%d:%d], %s, 0x0" % (CA, CA + 15, sp(SCP)))
    if ng == 10:
        a("s_load_dwordx4 s[%d:%d], %s, 0x40" % (CA + 16, CA + 19, sp(SCP)))
    a("s_sub_u32 s%d, %s, 1" % (SK, op["n"]))          # s80: steps behind the one at hand
    a("s_mov_b32 s%d, 0" % SK1)                        # s85: byte offset of the coefficient line last loaded
    if "head" in op:
        a("s_bfe_u32 s%d, %s, 0x70004" % (ST, op["head"]))        # e0: bits 4 .. 10 of the plan's header word (PlanSrc::head)
        a("s_lshl_b32 s%d, s%d, 2" % (ST, ST))
    else:
        a("s_lshl_b32 s%d, %s, 2" % (ST, op["e0"]))
    a("v_add_u32 v%d, s%d, %s" % (VN, ST, op["abase"]))           # v46: LDS address of position e0 of the lane's first sample: b[j-1] of step 0
    a("v_add_u32 v%d, 4, v%d" % (VN4, VN))
    L += reads(0, ng, K, VN4)            # bank 0 = b[j]
    L += reads(1, ng, K, VN)             # bank 1 = b[j-1]
    return L


def lines_regular(ng, K, rot, fused, op, end, jump_end):
    """op: the statement's operands by name (e0, or head: the plan's header word, which holds it); end: the label behind the routine,
    jump_end: it does not follow the text"""
    acc = ["%0", "%1", "%2", "%3", "%4", "%5"]
    L = prologue_regular(ng, K, op)
    a = L.append
    tail = []                            # the last step: out of line
    for r in range(2):
        H, Lb = r, 1 - r
        Cc, Cn = (CA, CB) if r == 0 else (CB, CA)
        a(".Lkiwi_rstep%d_%%=:" % r)
        a("s_waitcnt lgkmcnt(0)")
        a("s_sub_u32 s%d, s%d, 1" % (SK, SK))          # (the borrow: this is the last step)
        a("s_cbranch_scc1 .Lkiwi_rlast%d_%%=" % r)
        a("s_add_u32 s%d, s%d, %d" % (SK1, SK1, 80))
        a("s_load_dwordx16 s[%d:%d], %s, s%d" % (Cn, Cn + 15, sp(SCP), SK1))
        if ng == 10:
            a("s_load_dwordx4 s[%d:%d], %s, s%d offset:0x40" % (Cn + 16, Cn + 19, sp(SCP), SK1))
        a("v_add_u32 v%d, -4, v%d" % (VN, VN))         # the successor's shift is one more: its b[j-1] one position back
        L += arithmetic(ng, rot, fused, H, Lb, acc, K, True, C=Cc)
        if r == 1:
            a("s_branch .Lkiwi_rstep0_%=")
        tail.append(".Lkiwi_rlast%d_%%=:" % r)
        tail += arithmetic(ng, rot, fused, H, Lb, acc, C=Cc)
        if r == 0 or jump_end:
            tail.append("s_branch %s" % end)
    L += tail
    return L


def wrap_regular(name, L):
    text = "\\n\\t\"\n        \"".join(L)
    clob_v = ", ".join('"v%d"' % i for i in list(range(28, 44)) + [VN, VN4] + list(range(48, 128)))
    clob_s = ", ".join('"s%d"' % i for i in list(range(CA, CB + 20)) + [CLSL, CLSL + 1, SK, ST, SK1, SCP, SCP + 1])
    out = []
    out.append("__device__ __forceinline__ void %s(f2v &ar1a, f2v &ar1b, f2v &ar2a, f2v &ar2b, f2v &dza, f2v &dzb, unsigned abase, int e0,\n"
               "        int n, const float *coef, float cl, float sl)" % name)
    out.append("{")
    out.append('    asm volatile(\n        "%s\\n\\t"' % text)
    out.append('        : "+v"(ar1a), "+v"(ar1b), "+v"(ar2a), "+v"(ar2b), "+v"(dza), "+v"(dzb)')
    out.append('        : "v"(abase), "s"(e0), "s"(n), "s"(coef), "s"(cl), "s"(sl)')
    out.append('        : "memory", "scc", "vcc", %s,\n          %s);' % (clob_s, clob_v))
    out.append("}")
    return "\n".join(out)


def routine_plan(ng, K, rot, fused):
    """What accumulate_multi_kernel calls where it has plans: routine()'s text and routine_regular()'s in ONE statement, the choice
    between them a scalar bit test of the plan's header word (PlanSrc::head, bit 11: regular; bits 4 .. 10: e0) at its top.  (Two
    statements on the two sides of a C++ branch: the compiler either branches with a mask over the wave -- ten instructions per group
    -- or, for a scalar condition, copies the six accumulators in front of every statement and back behind it.)  Operands:
    routine()'s, then %13 the header word (s)."""
    name = "apply_plan_asm_%d_k%d_%s_%s" % (ng, K, "rot" if rot else "plain", "fused" if fused else "exact")
    L = ["s_bitcmp0_b32 %%13, %d" % 11, "s_cbranch_scc1 .Lkiwi_general_%="]
    L += lines_regular(ng, K, rot, fused, {"abase": "%6", "head": "%13", "n": "%9", "coef": "%10", "cl": "%11", "sl": "%12"}, ".Lkiwi_end_%=", True)
    L.append(".Lkiwi_general_%=:")
    L += lines_general(ng, K, rot, fused)          # (ends in its label .Lkiwi_end)
    return wrap_general(name, L, head=True)


REPEAT_BIT0 = 12                          # PlanSrc::head: bit 12 + j is set if record j + 1 of the group has record j's integer shift


def lines_repeat(ng, K, rot, fused, op, last, have_mask):
    """The apply of a group whose shifts grow by one OR STAY from step to step (bits 12 .. 15 of the plan's header word name the steps
    that stay: at most five steps).  routine_regular()'s text with a scalar test of the successor's bit in every step that has one:
      successor one sample on: the regular step -- its b[j-1] read behind this step's multiplies into the b[j] bank, the banks and the
        coefficient buffers swap (the other step text follows);
      successor at the SAME shift: its b[j] and b[j-1] are the two banks as they stand, so nothing is read.  The arithmetic runs without
        read-behind, the successor's coefficient line -- loaded into the other buffer at the top of this step -- is copied into the
        buffer at hand behind a wait, and the SAME step text runs again: banks, roles and buffers keep their parity.
    last: labels of the last-step bodies by parity (lines_regular()'s: a last step reads nothing ahead, whatever the group).
    have_mask: s84 holds the four bits already (the test at the statement's top).
    Registers as routine_regular()'s, and s84: the four bits (bit j: step j + 1 stays), s82: number of the successor's bit in them."""
    acc = ["%0", "%1", "%2", "%3", "%4", "%5"]
    L = prologue_regular(ng, K, op)
    a = L.append
    if not have_mask:
        a("s_bfe_u32 s%d, %s, 0x%x" % (SD, op["head"], 0x40000 | REPEAT_BIT0))
    a("s_mov_b32 s%d, -1" % SEN)
    tail = []                            # the steps whose successor repeats the shift: out of line, the regular path falls through
    for r in range(2):
        H, Lb = r, 1 - r
        Cc, Cn = (CA, CB) if r == 0 else (CB, CA)
        a(".Lkiwi_pstep%d_%%=:" % r)
        a("s_waitcnt lgkmcnt(0)")
        a("s_sub_u32 s%d, s%d, 1" % (SK, SK))          # (the borrow: this is the last step)
        a("s_cbranch_scc1 %s" % last[r])
        a("s_add_u32 s%d, s%d, %d" % (SK1, SK1, 80))
        a("s_load_dwordx16 s[%d:%d], %s, s%d" % (Cn, Cn + 15, sp(SCP), SK1))
        if ng == 10:
            a("s_load_dwordx4 s[%d:%d], %s, s%d offset:0x40" % (Cn + 16, Cn + 19, sp(SCP), SK1))
        a("s_add_u32 s%d, s%d, 1" % (SEN, SEN))
        a("s_bitcmp1_b32 s%d, s%d" % (SD, SEN))
        a("s_cbranch_scc1 .Lkiwi_prep%d_%%=" % r)
        a("v_add_u32 v%d, -4, v%d" % (VN, VN))
        L += arithmetic(ng, rot, fused, H, Lb, acc, K, True, C=Cc)
        if r == 1:
            a("s_branch .Lkiwi_pstep0_%=")
        t = tail.append
        t(".Lkiwi_prep%d_%%=:" % r)
        tail += arithmetic(ng, rot, fused, H, Lb, acc, C=Cc)
        t("s_waitcnt lgkmcnt(0)")                      # (the successor's coefficient line; no LDS read is in flight)
        for i in range(ng):
            t("s_mov_b64 %s, %s" % (sp(Cc + 2 * i), sp(Cn + 2 * i)))
        t("s_branch .Lkiwi_pstep%d_%%=" % r)
    return L + tail


def routine_steps(ng, K, rot, fused, one_text=False):
    """What accumulate_multi_kernel calls where it has plans, since the plans name the steps that repeat a shift: one statement, a
    three-way choice on the plan's header word at its top --
      bit 11 set                 lines_regular()'s text, as in routine_plan();
      a bit of 12 .. 15 set      lines_repeat()'s;
      neither                    lines_general()'s.
    one_text (A/B: `steps-one-text`, STEPS=steps-one-text of the Makefile): regular groups take lines_repeat()'s text too -- a mask of zero --, a test per
    step dearer, the statement four step bodies shorter.
    Operands: routine_plan()'s."""
    name = "apply_steps_asm_%d_k%d_%s_%s" % (ng, K, "rot" if rot else "plain", "fused" if fused else "exact")
    op = {"abase": "%6", "head": "%13", "n": "%9", "coef": "%10", "cl": "%11", "sl": "%12"}
    if one_text:
        L = ["s_and_b32 s%d, %%13, 0x%x" % (ST, (1 << 11) | (0xf << REPEAT_BIT0)), "s_cbranch_scc0 .Lkiwi_general_%="]
        L += lines_repeat(ng, K, rot, fused, op, [".Lkiwi_plast0_%=", ".Lkiwi_plast1_%="], False)
        for r in range(2):
            L.append(".Lkiwi_plast%d_%%=:" % r)
            L += arithmetic(ng, rot, fused, r, 1 - r, ["%0", "%1", "%2", "%3", "%4", "%5"], C=(CA, CB)[r])
            L.append("s_branch .Lkiwi_end_%=")
    else:
        L = ["s_bitcmp0_b32 %%13, %d" % 11, "s_cbranch_scc1 .Lkiwi_notregular_%="]
        L += lines_regular(ng, K, rot, fused, op, ".Lkiwi_end_%=", True)
        L.append(".Lkiwi_notregular_%=:")
        L += ["s_bfe_u32 s%d, %%13, 0x%x" % (SD, 0x40000 | REPEAT_BIT0), "s_cbranch_scc0 .Lkiwi_general_%="]       # (SCC: the field is not zero)
        L += lines_repeat(ng, K, rot, fused, op, [".Lkiwi_rlast0_%=", ".Lkiwi_rlast1_%="], True)
    L.append(".Lkiwi_general_%=:")
    L += lines_general(ng, K, rot, fused)          # (ends in its label .Lkiwi_end)
    return wrap_general(name, L, head=True)


if __name__ == "__main__":
    # no argument: kiwi_apply_asm.inc, the general routines.  `regular` / `plan` / `steps`: the routines of accumulate_multi_kernel's plans
    # (K = 17 is the grouped kernel's: no plan) -- `steps` is what the Makefile writes into build/kiwi_apply_steps_asm.inc
    family = sys.argv[1] if len(sys.argv) > 1 else "general"
    assert family in ("general", "regular", "plan", "steps", "steps-one-text")
    one_text = family == "steps-one-text"                 # (A/B: regular and repeating groups from one text, routine_steps)
    family = "steps" if one_text else family
    what = {"general": "the apply of one centroid group", "regular": "the apply of one REGULAR centroid group (shifts one apart: routine_regular)",
            "plan": "the apply of one centroid group, regular or not by the plan's header word (routine_plan)",
            "steps": "the apply of one centroid group: regular, with repeated shifts or general by the plan's header word (routine_steps)"}[family]
    print("// ---- (generated text: tools/gen_apply_asm.py%s) %s as a hand-allocated assembly routine" % ("" if family == "general" else " " + family, what))
    print("// KIWI_ARITH selects the exact (v_pk_mul_f32 + v_pk_add_f32) or the fused (v_pk_fma_f32) text")
    for fused in (False, True):
        print("#if KIWI_ARITH == %d" % (1 if fused else 0))
        for ng in (10, 8):
            for K in (5, 9, 17) if family == "general" else (5, 9):
                for rot in (True, False):
                    print({"general": routine, "regular": routine_regular, "plan": routine_plan,
                           "steps": lambda *a: routine_steps(*a, one_text=one_text)}[family](ng, K, rot, fused))
        print("#endif")
    print("// ---- (end of generated text)")
