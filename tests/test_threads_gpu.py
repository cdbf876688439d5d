"""The threading contract of include/tfa.h on the GPU: "the library keeps no state between calls except per-thread debug knobs", and the calling thread owns the
side streams of tfa_fwd_splitkv's chunk route.  A fixed list of small problems — one per family a serving loop calls — is run once serially on the default stream;
those results are held to their family's fp64 bounds (the helpers of the family's own GPU test, no new reference) and are then the expected BITS of
  * four Python threads, each under a torch.cuda.Stream of its own, every problem in two threads at once, ten repetitions on fresh copies of the inputs (ctypes
    releases the GIL: the library's host code overlaps; the same kernel instantiations, the same attr_mask and the CU-count cache are read from several threads,
    and each thread that takes the chunk route creates its own side-stream pool), and
  * one thread that interleaves two streams without host synchronisation, the chunk route twice back to back on both (one side-stream pool serves both).
The problems:
  1. fixed-length forward + backward: bf16, D 128, H4 / Hk2, causal, 320 x 385        fwd_ref bounds; form_ref.check_grads
  2. form_ref's varlen-w64_33, forward + backward, sequence by sequence               fwd_ref bounds per sequence; form_ref.check_grads per sequence
  3. kvcache_ref's two cases that append through kvcache_append_varlen(q=, rotary tables) into a paged cache — one with num_splits 2, one with an fp8 cache (no
     single case of the list is paged, fp8, appended AND split: the two together are)  kvcache_ref bounds; the caches and the rotated q against their definition
  4. a "-sched" case of kvcache_ref (get_scheduler_metadata)                           kvcache_ref bounds
  5. a kvcache_tree_ref case                                                           kvcache_ref bounds on kvcache_tree_ref's definition
  6. flash_attn_fwd_splitkv, B1 H8 Hk4 Nq3 Nk6000 D256, 4 splits: the chunk route      fwd_ref's split-KV bounds
  7. apply_rotary_emb on packed rows                                                   rotary_ref's bar
No graph is captured here (a capture's global mode and other threads' allocations do not mix).  The 60 s join limit is a hang guard far above any honest run — the
serial time of the list is printed next to it — not a timing assertion."""
import functools
import threading
import time
import traceback

import pytest
import torch

import form_ref as F
import fwd_ref as R
import kvcache_ref as K
import rotary_ref as RR
import test_boundary_gpu as TB
import test_forms_bwd_bounds_gpu as FB
import test_kvcache_fwd_bounds_gpu as KB
import test_kvcache_tree_gpu as TT

pytestmark = pytest.mark.gpu

THREADS, REPS, JOIN_LIMIT = 4, 10, 60.0
VARLEN_ID = "varlen-w64_33"
KV_APPEND_IDS = ("vq-append-bf16-d64-g2-causal-page128-s2", "vq-append-fp8-fp16-d48-g2-causal-page64")
KV_SCHED_ID = "vq-fp8-fp16-d112-g2-causal-page256-pack-sched"
TREE_ID = "t4d-bf16-d104-g4-nq33-page128-s3-pack"
_hung = []                       # a thread that outlived the join limit: nothing in this module touches the GPU afterwards


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def cpu(*xs):
    return [x.cpu() for x in xs]


def same_bits(a, b):
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


# ---- the problems: run(dev) -> [CPU tensors] on the current stream from fresh device copies; check(outs): the family's fp64 bounds ------------------------
@functools.lru_cache(maxsize=None)
def fwd_reference(case_id):
    t = R.build(R.BOUNDARY_BY_ID[case_id])
    return t, R.reference(t)[None]


def run_fixed(dev):
    from tiny_flash_attention_amd import ops

    t, _ = fwd_reference(R.THREADS_CASE["id"])
    q, k, v, do = (t[n].to(dev) for n in ("q", "k", "v", "dout"))
    o, l = ops.flash_attn_fwd(q, k, v, True, t["sc"])
    g16 = ops.flash_attn_bwd(q, k, v, o, l, do, True, t["sc"])
    g32 = ops.flash_attn_bwd(q, k, v, o, l, do, True, t["sc"], grad_f32=True)
    return cpu(o, l, *g16, *g32)


def check_fixed(outs):
    t, ref = fwd_reference(R.THREADS_CASE["id"])
    o, l, g16, g32 = outs[0], outs[1], outs[2:5], outs[5:8]
    TB.hold_to_bounds(t["case"]["id"], t, ref, o, l, False)
    part = (t["q"], t["k"], t["v"], t["dout"], t["form"])
    grads = (F.ref_grads(t["q"], t["k"], t["v"], t["dout"], t["sc"], **t["form"]), F.structure(t["q"], t["k"], t["sc"], **t["form"]))
    FB.check_part(t["case"]["id"], g32, g16, o, part, grads, t["sc"], t["dtype"])


def run_varlen(dev):
    from tiny_flash_attention_amd import ops

    t, _, _ = FB.reference(VARLEN_ID)
    c, sc = t["case"], t["sc"]
    q, k, v, do = (t[n].to(dev) for n in ("q", "k", "v", "dout"))
    cu, kw = FB.varlen_args(t, dev)
    o, l = ops.flash_attn_varlen_fwd(q, k, v, *cu, c["causal"], sc, out=torch.zeros_like(q), **kw)
    g16 = ops.flash_attn_varlen_bwd(q, k, v, o, l, do, *cu, c["causal"], sc, **kw)
    g32 = ops.flash_attn_varlen_bwd(q, k, v, o, l, do, *cu, c["causal"], sc, grad_f32=True, **kw)
    l = l[:, :int(t["cu_q"][-1])]                           # (the LSE of the rows outside every sequence is never written: whatever the allocation held)
    return cpu(o, l, *g16, *g32)


def check_varlen(outs):
    t, parts, refs = FB.reference(VARLEN_ID)
    c, cq = t["case"], t["cu_q"]
    o, l, g16, g32 = outs[0], outs[1], outs[2:5], outs[5:8]
    FB.check_packed(VARLEN_ID, t, parts, refs, o, g32, g16)
    for b, (q, k, v, _, f) in parts.items():               # the forward, sequence by sequence
        if b not in refs:
            continue
        o64, l64, A = F.ref_fwd(q, k, v, t["sc"], **f)
        T = R.bound_terms(q, k, t["sc"], **f)
        bound = R.lse_bound(T, k.shape[2], torch.where(torch.isfinite(l64), l64, torch.zeros_like(l64)), c["D"], slopes=c["slopes"] is not None, cap=c["cap"])
        lse = l[:, int(cq[b]):int(cq[b + 1])].unsqueeze(0)
        TB.hold_to_bounds(f"{VARLEN_ID}[seq {b}]", t, (o64, l64, A, T, bound), F.seq_view(o, cq, b), lse, False)


def flat(res):
    return [x for b in sorted(res) for x in res[b]]


def check_kvcache(case_id, t, ref, outs):
    """tests/test_kvcache_fwd_bounds_gpu.py's assertions on a result that is already there."""
    c = t["case"]
    got = dict(zip(sorted(ref), zip(outs[0::2], outs[1::2])))
    assert len(outs) == 2 * len(ref)
    wo = wl = 0.0
    for b, (out, lse, A, T, n) in ref.items():
        o, l = got[b]
        assert not bool(torch.isnan(o).any()) and not bool(torch.isnan(l).any()), f"{case_id}[seq {b}]: NaN"
        unseen = torch.isposinf(lse)
        assert torch.equal(torch.isposinf(l), unseen) and bool((o.transpose(0, 1)[unseen] == 0).all()), f"{case_id}[seq {b}]: rows that see no key"
        wo, wl = max(wo, K.out_ratio(o.double(), out, A, t["dtype"])), max(wl, K.lse_ratio(l, lse, T, n, c["D"], K.lse_splits(c)))
    print(f"{case_id}: max(|d| / bound) out {wo:.3f}  lse {wl:.4f}")
    assert wo <= 1.0 and wl <= 1.0, f"{case_id}: out at {wo:.3f}, lse at {wl:.3f} of their per-element bounds"


def kv_item(case_id):
    def run(dev):
        return flat(KB.call(KB.reference(case_id)[0], dev))            # (call asserts the caches and the rotated q against what the append is defined to store)

    def check(outs):
        t, ref = KB.reference(case_id)
        check_kvcache(case_id, t, ref, outs)

    return case_id, run, check


def run_tree(dev):
    return flat(TT.call(TT.reference(TREE_ID)[0], dev))


def check_tree(outs):
    t, ref = TT.reference(TREE_ID)
    TT.check(TREE_ID, t, ref, dict(zip(sorted(ref), zip(outs[0::2], outs[1::2]))))


def run_splitkv(dev):
    from tiny_flash_attention_amd import ops

    t, _ = fwd_reference(R.THREADS_SPLITKV_CASE["id"])
    c = t["case"]
    o, l = ops.flash_attn_fwd_splitkv(t["q"].to(dev), t["k"].to(dev), t["v"].to(dev), c["causal"], t["sc"], splits=c["splits"])
    return cpu(o, l)


def check_splitkv(outs):
    t, ref = fwd_reference(R.THREADS_SPLITKV_CASE["id"])
    TB.hold_to_bounds(t["case"]["id"], t, ref, outs[0], outs[1], False)


@functools.lru_cache(maxsize=None)
def rotary_problem():
    """tests/test_rotary_gpu.py's packed form: lengths [0, 1, 65, 7] and 3 rows outside every sequence, x a slice of a packed projection."""
    lens, pad, H, D, rd, off = [0, 1, 65, 7], 3, 3, 128, 32, [5, 0, 20, 78]
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    total = cu[-1] + pad
    buf = torch.empty((total, 3, H, D)).normal_(0.0, 1.0, generator=torch.Generator().manual_seed(160)).to(torch.bfloat16)
    cos, sin = RR.tables(80, rd, torch.float32)
    pos, valid = RR.packed_positions(total, cu, off)
    return dict(buf=buf, cos=cos, sin=sin, cu=cu, off=off, pos=pos, valid=valid, max_len=max(lens))


def run_rotary(dev):
    import tiny_flash_attention_amd as tfa

    p = rotary_problem()
    bufd = p["buf"].to(dev)
    out = tfa.apply_rotary_emb(bufd[:, 1], p["cos"].to(dev), p["sin"].to(dev), seqlen_offsets=torch.tensor(p["off"], dtype=torch.int32, device=dev),
                               cu_seqlens=torch.tensor(p["cu"], dtype=torch.int32, device=dev), max_seqlen=p["max_len"])
    return cpu(out)


def check_rotary(outs):
    p = rotary_problem()
    x = p["buf"][:, 1]
    ref, mag, rotated = RR.rotary_ref64(x, p["cos"], p["sin"], p["pos"], False, False, p["valid"])
    e = RR.excess(outs[0], ref, mag, torch.bfloat16)
    print(f"rotary packed rows: the worst element is {e:.3e} above ulp/2 + 2^-21 (|x1| + |x2|) (<= 0 passes)")
    assert e <= 0.0 and bool(rotated.any()) and not bool(rotated[-3:].any())
    assert same_bits(outs[0][~rotated], x[~rotated].contiguous()), "an unrotated row is not a bit-for-bit copy"


ITEMS = [("fixed fwd+bwd", run_fixed, check_fixed), ("varlen fwd+bwd", run_varlen, check_varlen), kv_item(KV_APPEND_IDS[0]), kv_item(KV_APPEND_IDS[1]),
         kv_item(KV_SCHED_ID), ("tree " + TREE_ID, run_tree, check_tree), ("splitkv chunk route", run_splitkv, check_splitkv), ("rotary packed", run_rotary, check_rotary)]
# every problem in two threads, which run it in the same order: threads 0 and 1 the even entries, 2 and 3 the odd ones
ASSIGN = [ITEMS[0::2], ITEMS[0::2], ITEMS[1::2], ITEMS[1::2]]
_serial = {}


def serial_results(dev):
    """Every problem once on the default stream: held to its family's fp64 bounds, then the expected bits.  (Cached once it has passed.)"""
    if not _serial:
        assert not _hung, "an earlier test of this module left a thread running: the GPU is not touched again"
        res = {}
        for name, run, _ in ITEMS:                          # (untimed: the first call of a kernel loads its code object and builds the CPU references)
            res[name] = run(dev)
        t0 = time.perf_counter()
        again = {name: run(dev) for name, run, _ in ITEMS}
        torch.cuda.synchronize()
        res["seconds"] = time.perf_counter() - t0
        for name, _, check in ITEMS:
            check(res[name])
            assert all(same_bits(a, b) for a, b in zip(res[name], again[name])), f"{name}: two serial runs differ in bits"
        _serial.update(res)
    return _serial


def test_four_threads_four_streams(dev):
    want = serial_results(dev)
    budget = want["seconds"] * REPS * max(len(a) for a in ASSIGN) / len(ITEMS)
    print(f"serial time of the work list: {want['seconds']:.3f} s; a thread's share, {REPS} times: {budget:.2f} s; join limit (hang guard): {JOIN_LIMIT:.0f} s")
    barrier = threading.Barrier(THREADS)
    results, errors = [[] for _ in range(THREADS)], []

    def work(i):
        try:
            stream = torch.cuda.Stream(device=dev)
            barrier.wait(timeout=JOIN_LIMIT)
            with torch.cuda.stream(stream):
                for rep in range(REPS):
                    for name, run, _ in ASSIGN[i]:
                        results[i].append((name, rep, run(dev)))
                stream.synchronize()
        except BaseException:                               # noqa: BLE001  (reported with its traceback below)
            errors.append(f"thread {i}:\n{traceback.format_exc()}")

    threads = [threading.Thread(target=work, args=(i,), daemon=True, name=f"tfa-worker-{i}") for i in range(THREADS)]
    t0 = time.perf_counter()
    for th in threads:
        th.start()
    deadline = t0 + JOIN_LIMIT
    for th in threads:
        th.join(max(0.0, deadline - time.perf_counter()))
    alive = [th.name for th in threads if th.is_alive()]
    if alive:
        _hung.append(alive)
        pytest.fail(f"{alive} still running after {JOIN_LIMIT:.0f} s (serial time of the list: {want['seconds']:.3f} s): a hang; the GPU is not touched again")
    print(f"{THREADS} threads x {REPS} repetitions: {time.perf_counter() - t0:.2f} s")
    assert not errors, "\n".join(errors)
    for i in range(THREADS):
        assert len(results[i]) == REPS * len(ASSIGN[i])
        for name, rep, outs in results[i]:
            assert len(outs) == len(want[name]) and all(same_bits(a, b) for a, b in zip(outs, want[name])), \
                f"thread {i}, repetition {rep}, {name}: not the serial result's bits"


def test_one_thread_two_streams(dev):
    """A's forward on s1, B on s2, A's backward on s1, B again on s2 — no host synchronisation in between — then the chunk route back to back on s1 and s2: the
    calling thread's one side-stream pool serves both.  A = problem 1, B = problem 6."""
    from tiny_flash_attention_amd import ops

    want = serial_results(dev)
    assert not _hung, "an earlier test of this module left a thread running: the GPU is not touched again"
    ta, _ = fwd_reference(R.THREADS_CASE["id"])
    tb, _ = fwd_reference(R.THREADS_SPLITKV_CASE["id"])
    q, k, v, do = (ta[n].to(dev) for n in ("q", "k", "v", "dout"))
    qb, kb, vb = (tb[n].to(dev) for n in ("q", "k", "v"))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    split = lambda: ops.flash_attn_fwd_splitkv(qb, kb, vb, True, tb["sc"], splits=tb["case"]["splits"])      # noqa: E731
    with torch.cuda.stream(s1):
        o, l = ops.flash_attn_fwd(q, k, v, True, ta["sc"])
    with torch.cuda.stream(s2):
        b1 = split()
    with torch.cuda.stream(s1):
        g16 = ops.flash_attn_bwd(q, k, v, o, l, do, True, ta["sc"])
        g32 = ops.flash_attn_bwd(q, k, v, o, l, do, True, ta["sc"], grad_f32=True)
    with torch.cuda.stream(s2):
        b2 = split()
    with torch.cuda.stream(s1):
        b3 = split()
    with torch.cuda.stream(s2):
        b4 = split()
    torch.cuda.synchronize()
    got_a = cpu(o, l, *g16, *g32)
    assert all(same_bits(x, y) for x, y in zip(got_a, want["fixed fwd+bwd"])), "problem 1 interleaved with the chunk route on another stream: not the serial bits"
    for n, b in enumerate((b1, b2, b3, b4)):
        assert all(same_bits(x, y) for x, y in zip(cpu(*b), want["splitkv chunk route"])), f"chunk-route call {n + 1} of 4 on two streams: not the serial bits"
