"""CPU: a model of the step schedule of conv3x3_split_kernel (csrc/conv_split3x3.hip), so that a race cannot pass by luck on
small images.  The schedule's constants -- the staging steps SB / SA / LA / LB, the entries per thread NEK, the tap count, where
the step's barrier sits and what the weight DMA targets -- are read from the source, so the model cannot drift from the kernel.

The model replays the program of one wave (all eight run the same one) over the prologue and three periods and records every
access to the four LDS regions -- input buffer 0 / 1: B-fragment reads by tap unit, staging stores; weight slot 0 / 1: A-fragment
reads including the pre-read for the next step, DMA issue and DMA wait -- each with the number of barriers the wave has passed when
the access is issued and when it is complete (a read: at its first use or at the LDS wait in front of a barrier; a store: at that
wait; a DMA: at the wave's vmcnt(0)).  Between waves only barriers order, so a region is safe when every write of content v is
issued after a barrier that follows the completion of every read of content v - 1, and complete before a barrier that precedes the
issue of every read of content v.  Beside that: no staging register set is loaded before its previous value was stored.

Negative case: the boundary-barrier schedule combined with the pre-read (the timing-only ablation of DESIGN.md section 9.1) reads
a slice in the step its DMA is still landing in -- the model must reject it."""
import os
import re
from dataclasses import dataclass

import pytest

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cwfa_amd", "csrc", "conv_split3x3.hip")


def _kernel_source():
    s = open(SRC).read()
    a = s.index("void conv3x3_split_kernel(SParams p)")
    return s[:a], s[a:s.index("namespace few")]


def parse():
    """the schedule's constants as the source states them"""
    head, k = _kernel_source()
    m = re.search(r"constexpr int SB = (\d+), SA = KS == 3 \? (\d+) : (\d+), LA = KS == 3 \? (\d+) : (\d+), LB = KS == 3 \? (\d+) : (\d+);", k)
    sb, sa3, sa7, la3, la7, lb3, lb7 = map(int, m.groups())
    nek2, nek3 = map(int, re.search(r"NEK = SPECIAL \? (\d+) : (\d+);", head).groups())
    assert re.search(r"SPECIAL = KS == 3 && RPW == 4;", head) and re.search(r"NTAP = KS \* KS", head)
    assert re.search(r"constexpr int MID = NT / 2;", k), "barrier position"
    assert re.search(r"constexpr bool MIDSTEP = !ADD;", k)
    assert re.search(r"LOAD_NT = MIDSTEP \? MID : 0, DMA_NT = !MIDSTEP \? 1 : NT >= 8 \? MID \+ 1 : MID;", k)
    assert re.search(r"if \(MIDSTEP && nt == MID - 1\) \{", k) and re.search(r"if \(MIDSTEP && nt == NT - 1 && mt < MA\) \{", k)
    assert re.search(r"if constexpr \(MIDSTEP\) dma_w\(step \+ 2, sl\);", k) and re.search(r"else dma_w\(step \+ 1, sl \^ 1\);", k)
    assert re.search(r"if constexpr \(MIDSTEP\) dma_w\(1, 1\);", k), "prologue: slice 1"
    assert re.search(r"if \(MIDSTEP && nt == NT - 1\) read_b_next\(\);", k) and re.search(r"if constexpr \(!MIDSTEP\) read_b_next\(\);", k)
    assert re.search(r"constexpr int NB = MPW == 4 \? 3 : 2, MA = MPW == 4 \? 2 : MPW;", k)
    return {3: dict(SB=sb, SA=sa3, LA=la3, LB=lb3, NTAP=9, NEK={True: nek2, False: nek3}),
            7: dict(SB=sb, SA=sa7, LA=la7, LB=lb7, NTAP=49, NEK={True: nek3, False: nek3})}


@dataclass(frozen=True)
class Form:
    ks: int
    special: bool             # 3x3 on 8-row tiles: two staging entries per thread
    nt: int                   # n-tiles per wave
    mpw: int
    midstep: bool             # barrier in the middle of the step (kernel: !ADD)
    preread: bool             # the next step's A fragments are requested inside the last n-tile (kernel: == midstep)


@dataclass
class Ev:
    region: str
    kind: str                 # "r" | "w"
    version: int
    issue: int                # barriers passed at issue
    done: int                 # barriers passed when complete
    what: str


def simulate(f, const, periods=3):
    """-> (LDS events, register-set log) of one wave over the prologue and `periods` periods"""
    c = const[f.ks]
    SB, SA, LA, LB, NTAP, NEK = c["SB"], c["SA"], c["LA"], c["LB"], c["NTAP"], c["NEK"][f.special]
    NT, MPW = f.nt, f.mpw
    NB, MA = (3, 2) if MPW == 4 else (2, MPW)
    MID = NT // 2
    LOAD_NT = MID if f.midstep else 0
    DMA_NT = 1 if not f.midstep else MID + 1 if NT >= 8 else MID
    ev, regs = [], []
    epoch = 0
    pend_dma, pend_lds = [], []          # events whose completion is the next vmcnt(0) / the next LDS wait or use

    def lds_wait(keep=0):                # the wave's LDS wait in front of a barrier: everything but the youngest `keep` reads
        done = pend_lds[:len(pend_lds) - keep] if keep else pend_lds[:]
        for e in done:
            e.done = epoch
            pend_lds.remove(e)

    def use(e):                          # first use of a read's registers
        if e in pend_lds:
            e.done = epoch
            pend_lds.remove(e)

    def add(region, kind, version, what, pend):
        e = Ev(region, kind, version, epoch, None, what)
        ev.append(e)
        pend.append(e)
        return e

    def b_reads(step):
        """(region, version) of the B fragments of a step: its two tap units"""
        q, P = divmod(step, NTAP)
        out = []
        for u in (2 * P, 2 * P + 1):
            out.append(("buf1", 2 * q + 1) if u >= NTAP else ("buf0", 2 * q))
        return out

    def read_b(step, nt):
        return [add(r, "r", v, f"B step {step} n-tile {nt}", pend_lds) for r, v in b_reads(step)]

    # ---- prologue: chunk 0 stored, chunk 1 loaded into the set, slice 0 (MIDSTEP: and 1) by DMA, full drain, barrier
    for k in range(NEK):
        regs.append((k, "load", 1))
        add("buf0", "w", 0, f"prologue store entry {k}", pend_lds)
    add("slot0", "w", 0, "DMA slice 0", pend_dma)
    if f.midstep:
        add("slot1", "w", 1, "DMA slice 1", pend_dma)
    for e in pend_dma:
        e.done = epoch
    pend_dma.clear()
    lds_wait()
    epoch += 1
    a_lo = [add("slot0", "r", 0, "A[0..MA) step 0", pend_lds)] if f.preread else None
    b0 = read_b(0, 0)

    def staging_stores(step):
        q, P = divmod(step, NTAP)
        for k in range(NEK):
            if P == SB + k:
                regs.append((k, "store", 2 * q + 1))
                add("buf1", "w", 2 * q + 1, f"store entry {k} step {step}", pend_lds)
            if P == SA + k:
                regs.append((k, "store", 2 * q + 2))
                add("buf0", "w", 2 * q + 2, f"store entry {k} step {step}", pend_lds)

    for step in range(periods * NTAP):
        q, P = divmod(step, NTAP)
        slot, nslot = f"slot{step & 1}", f"slot{(step + 1) & 1}"
        if not f.midstep:
            staging_stores(step)
        if not f.preread:
            a_lo = [add(slot, "r", step, f"A[0..MA) step {step}", pend_lds)]
        bq = {0: b0}
        a_next = None
        for nt in range(NT):
            if (MA == MPW or nt > 0) and nt + NB - 1 < NT:
                bq[nt + NB - 1] = read_b(step, nt + NB - 1)
            if f.midstep and nt == NT - 1:           # the next step's first B fragments: in front of the last n-tile
                b0 = read_b(step + 1, 0)
            for mt in range(MPW):
                for e in bq[nt] + (a_lo if mt < MA else a_hi):
                    use(e)
                if MA < MPW and nt == 0 and mt == 0:
                    a_hi = [add(slot, "r", step, f"A[MA..MPW) step {step}", pend_lds)]
                    for n2 in range(1, min(NB, NT)):
                        bq[n2] = read_b(step, n2)
                if f.preread and nt == NT - 1 and mt == MA - 1:
                    a_next = [add(nslot, "r", step + 1, f"A[0..MA) step {step + 1} (pre-read)", pend_lds)]
            if f.midstep and nt == MID - 1:
                for e in pend_dma:
                    e.done = epoch
                pend_dma.clear()
                lds_wait(keep=2 * (NB - 1))          # (two tap units per set)
                epoch += 1
                staging_stores(step)
            if nt == LOAD_NT:
                for k in range(NEK):
                    if P == LA + k:
                        regs.append((k, "load", 2 * q + 2))
                    if P == LB + k:
                        regs.append((k, "load", 2 * q + 3))
            if nt == DMA_NT:
                if f.midstep:
                    add(slot, "w", step + 2, f"DMA slice {step + 2}", pend_dma)
                else:
                    add(nslot, "w", step + 1, f"DMA slice {step + 1}", pend_dma)
        if not f.midstep:                            # boundary barrier: in front of it
            b0 = read_b(step + 1, 0)
        if f.preread:
            a_lo = a_next
        if not f.midstep:
            for e in pend_dma:
                e.done = epoch
            pend_dma.clear()
            lds_wait(keep=2 + (1 if f.preread else 0) * 0)    # the B reads just issued stay outstanding (the pre-read A is older: waited)
            epoch += 1
    for e in ev:                                 # whatever is still outstanding at the end completes after the last barrier
        if e.done is None:
            e.done = epoch
    return ev, regs


def hazards(ev):
    bad = []
    for region in ("buf0", "buf1", "slot0", "slot1"):
        es = [e for e in ev if e.region == region]
        versions = sorted({e.version for e in es if e.kind == "w"})
        for w in (e for e in es if e.kind == "w"):
            i = versions.index(w.version)
            for r in (e for e in es if e.kind == "r"):
                if i > 0 and r.version == versions[i - 1] and not r.done < w.issue:
                    bad.append(("write after read", region, w.what, r.what))
                if r.version == w.version and not r.issue > w.done:
                    bad.append(("read after write", region, w.what, r.what))
        assert all(e.version in versions for e in es if e.kind == "r"), (region, "a read of content that was never written")
    return bad


def register_sets(regs):
    """per entry: load, store, load, store, ... of the same chunk"""
    bad = []
    for k in {k for k, _, _ in regs}:
        seq = [(op, ch) for kk, op, ch in regs if kk == k]
        for i, (op, ch) in enumerate(seq):
            if op != ("load", "store")[i & 1] or (op == "store" and ch != seq[i - 1][1]):
                bad.append((k, i, seq[max(0, i - 2):i + 1]))
                break
    return bad


# the kernel's forms: (KS, two-entry staging map, n-tiles per wave, m-tiles per wave, skip add)
KERNEL_FORMS = [(3, True, 8, 4, False), (3, True, 8, 4, True), (3, True, 8, 2, False), (3, True, 8, 2, True), (3, True, 8, 1, False),
                (3, True, 8, 1, True), (3, False, 8, 2, False), (3, False, 8, 3, False), (3, False, 8, 1, False), (3, False, 4, 3, False),
                (3, False, 4, 2, False), (3, False, 4, 1, False), (7, False, 4, 2, False)]


@pytest.mark.parametrize("ks,special,nt,mpw,add", KERNEL_FORMS)
def test_schedule_of_every_form_is_race_free(ks, special, nt, mpw, add):
    const = parse()
    f = Form(ks, special, nt, mpw, midstep=not add, preread=not add)
    ev, regs = simulate(f, const)
    assert not hazards(ev), hazards(ev)[:4]
    assert not register_sets(regs), register_sets(regs)
    # every region is exercised: both buffers and both slots are written and read in every period
    for region in ("buf0", "buf1", "slot0", "slot1"):
        assert sum(e.region == region and e.kind == "w" for e in ev) >= 3 and any(e.region == region and e.kind == "r" for e in ev)


def test_source_constants():
    c = parse()
    assert c[3]["NTAP"] == 9 and c[7]["NTAP"] == 49 and c[3]["NEK"] == {True: 2, False: 3}
    for ks in (3, 7):
        k = c[ks]
        assert k["SB"] < k["LA"] and k["SA"] <= k["LB"] and k["LB"] + 3 - 1 < k["NTAP"]


@pytest.mark.parametrize("ks,special,nt,mpw", [(3, True, 8, 4), (3, False, 4, 3), (7, False, 4, 2)])
def test_preread_with_the_boundary_barrier_is_rejected(ks, special, nt, mpw):
    """the ablation: the barrier stays at the step boundary and the next step's A fragments are read inside the last n-tile, from
    the slot its slice is still landing in"""
    ev, _ = simulate(Form(ks, special, nt, mpw, midstep=False, preread=True), parse())
    bad = hazards(ev)
    assert bad and all(b[0] == "read after write" and b[1].startswith("slot") and "pre-read" in b[3] for b in bad), bad[:4]


def test_model_sees_a_store_in_the_wrong_half():
    """the model is sensitive to the staging steps: the even buffer written one step early (while tap NTAP-1 is still read) and
    the odd buffer completed one step late are both found"""
    const = parse()
    f = Form(3, False, 8, 2, midstep=True, preread=True)
    early = {3: dict(const[3], SA=const[3]["SA"] - 1, LA=const[3]["LA"] - 1), 7: const[7]}
    assert any(b[0] == "write after read" and b[1] == "buf0" for b in hazards(simulate(f, early)[0]))
    late = {3: dict(const[3], SB=const[3]["SB"] + 1, LA=const[3]["LA"] + 1, SA=const[3]["SA"] + 1, LB=const[3]["LB"]), 7: const[7]}
    assert any(b[0] == "read after write" and b[1] == "buf1" for b in hazards(simulate(f, late)[0]))
