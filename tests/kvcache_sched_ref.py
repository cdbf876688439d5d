"""Host restatements for the tests of the scheduled packed-q K/V-cache call (include/tfa.h: tfa_kvcache_varlen_schedule, tfa_fwd_kvcache_varlen_sched): the work
list as the schedule kernel writes it, the bound as the header states it, the attention kernel's decode of a list entry with its clamps, and the lists that do NOT
belong to a batch which the clamping tests feed to both."""
import random

HDR = 8                 # header words: n_items, B, G', causal, max_seqlen_q, total_q, bound, 0
BM = 128                # rows of a query block
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


# the batch of the GPU clamping test (tests/test_kvcache_sched_gpu.py::test_clamping): tests/test_kvcache_varlenq_gpu.py's ragged rows, two rows of no sequence
# in front of cu[0] and three behind cu[B]; and the rows of another batch of the same B whose list is fed to it
CLAMP_NQ, CLAMP_MAXQ, CLAMP_OTHER_NQ = [1, 0, 7, 1, 40, 1, 5], 40, [40, 1, 0, 0, 2, 7, 5]
CLAMP_CU = [2, 3, 3, 10, 11, 51, 52, 57]
CLAMP_TOTAL_Q = 60


def rows_of(cu, total_q, max_q):
    """(q0_b, nq_b) as every work item clamps them (include/tfa.h)."""
    res = []
    for b in range(len(cu) - 1):
        q0 = min(max(int(cu[b]), 0), total_q)
        res.append((q0, min(max(int(cu[b + 1]) - int(cu[b]), 0), min(max_q, total_q - q0))))
    return res


def blocks_of(nq, gp):
    return (nq * gp + BM - 1) // BM


def items_of(nb, causal):
    return (nb + 1) // 2 if causal else nb


def bound_of(B, max_q, total_q, gp, causal):
    """The header's bound: not causal min(B * nmb, F + B), causal min(B * ceil(nmb / 2), (F + 2 B) // 2); F = ceil(total_q * G' / 128)."""
    nmb = blocks_of(max_q, gp)
    F = (total_q * gp + BM - 1) // BM
    if causal and nmb > 1:
        return min(B * ((nmb + 1) // 2), (F + 2 * B) // 2)
    return min(B * nmb, F + B)


def schedule(cu, max_q, total_q, gp, causal):
    """header + the item rows that are written (a flat list of ints): ascending b, then ascending wi; the list ends at the bound."""
    B = len(cu) - 1
    bound = bound_of(B, max_q, total_q, gp, causal)
    rows = []
    for b, (_, nq) in enumerate(rows_of(cu, total_q, max_q)):
        rows += [(b, wi) for wi in range(items_of(blocks_of(nq, gp), causal))]
    rows = rows[:bound]
    return [len(rows), B, gp, 1 if causal else 0, max_q, total_q, bound, 0] + [x for r in rows for x in r]


def decode(meta, cu, max_q, total_q, gp, causal):
    """The attention kernel's decode of every index of the launch (tfa_fwd_kernel_dma_body.inc, the SCHED statements), clamps included: the (sequence, block)
    pairs that run.  Asserts what the kernel relies on: every read of the list lies inside its HDR + 2 * bound entries, every pair is a block of its sequence."""
    B = len(cu) - 1
    bound = bound_of(B, max_q, total_q, gp, causal)
    assert len(meta) <= HDR + 2 * bound
    meta = list(meta) + [0] * (HDR + 2 * bound - len(meta))      # (schedule() returns the written words only: the rest of the buffer is whatever it held)
    seqs = rows_of(cu, total_q, max_q)
    n_items = min(max(int(meta[0]), 0), bound)
    touched = []
    for si in range(bound):
        if si >= n_items:                                # behind the list's end: the workgroup returns
            continue
        assert HDR + 2 * si + 1 < len(meta)
        b, wi = int(meta[HDR + 2 * si]), int(meta[HDR + 2 * si + 1])
        b0 = min(max(b, 0), B - 1)
        nb = blocks_of(seqs[b0][1], gp)
        if wi < 0 or wi >= items_of(nb, causal):         # none of the sequence's own items: an item without rows
            continue
        mbs = [nb - 1 - wi] + ([wi] if nb - 1 - wi != wi else []) if causal else [wi]
        for mb in mbs:
            assert 0 <= b0 < B and 0 <= mb < nb and mb * BM < seqs[b0][1] * gp, (b, wi, b0, mb, nb)
            touched.append((b0, mb))
    return touched


def foreign_lists(cu, max_q, total_q, gp, causal, other_nq):
    """Lists that do not belong to the batch, each HDR + 2 * bound int32 values: built for other row counts (other_nq: the same B and total), n_items far above
    the bound over random rows, negative and huge (b, wi), duplicated rows, random words."""
    B = len(cu) - 1
    bound = bound_of(B, max_q, total_q, gp, causal)
    size = HDR + 2 * bound
    rng = random.Random(1234)
    own = schedule(cu, max_q, total_q, gp, causal)
    pad = lambda m: (m + [0] * size)[:size]
    res = {}
    ocu = [0]
    for n in other_nq:
        ocu.append(ocu[-1] + n)
    assert len(ocu) == B + 1 and ocu[-1] <= total_q
    res["other row counts"] = pad(schedule(ocu, max_q, total_q, gp, causal))
    huge = pad(list(own))
    huge[0] = I32_MAX
    for i in range(HDR + 2 * own[0], size):
        huge[i] = rng.randrange(-3, B + 3)
    res["n_items far above the bound"] = huge
    bad_b = [-5, I32_MAX, I32_MIN, B, B + 100, -1, 0, B - 1]
    bad_wi = [-1, I32_MIN, I32_MAX, 1000, 0, 1, 2, -7]
    m = [bound, B, gp, 1 if causal else 0, max_q, total_q, bound, 0]
    for i in range(bound):
        m += [bad_b[i % len(bad_b)], bad_wi[(i // 2) % len(bad_wi)]]
    res["negative and huge rows"] = m
    busiest = max(range(B), key=lambda b: rows_of(cu, total_q, max_q)[b][1])
    res["duplicated rows"] = [bound, B, gp, 1 if causal else 0, max_q, total_q, bound, 0] + [busiest, 0] * bound
    res["negative n_items"] = pad([-3] + own[1:])
    res["random words"] = [rng.randrange(I32_MIN, I32_MAX + 1) for _ in range(size)]
    for m in res.values():
        assert len(m) == size and all(I32_MIN <= x <= I32_MAX for x in m)
    return res
