"""Records what every host-only K/V-cache entry point of the C ABI answers over a grid of calls: tests/golden/kvcache_host_answers.json.

    TFA_LIB=<a build of the commit to record>/libtfa_hip.so python tests/golden/make_kvcache_host_answers.py

The file holds a list of cases, each the description of one call (only the fields that differ from DEFAULTS) and the answers of ALL entry points in ENTRY_POINTS to
it, in that order: the status and (grid, block, lds) of a _plan, the fp32 words (or the status) of a _workspace, the chunk count of a _suggest_splits, the int32 words
of tfa_kvcache_varlen_schedule_size.  tests/test_kvcache_host_answers_cpu.py replays every case against the built library and compares answer by answer.  Nothing
here touches a GPU: plans never launch and never read the stand-in pointers.  The suggestions assume 256 CUs: what the library answers without a device, and an MI355X.
"""
import ctypes as C
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tiny_flash_attention_amd import _lib  # noqa: E402

OUT = os.path.join(HERE, "kvcache_host_answers.json")
ADDR = 0x10000                      # a 16-byte aligned stand-in for device pointers
POINTERS = ("q", "out", "lse", "k_cache", "v_cache", "cache_seqlens", "block_table", "cu_seqlens_q", "tree_mask", "k_descale", "v_descale")
# one call: the problem, the cache, the chunking and packing, the q layout, the rider — and `mut`, named edits of the finished structs (mutate below)
DEFAULTS = dict(dtype=_lib.TFA_BF16, D=64, B=3, H=8, Hk=2, Nq=5, cap=1024, page=0, splits=1, pack=0, causal=1, fp8=0, vq=None, left=-1, sched=0, tree=0, mut=())
ENTRY_POINTS = (
    "kvcache_plan", "kvcache_workspace", "kvcache_suggest_splits", "fp8_plan", "fp8_workspace", "pack_plan", "pack_workspace", "pack_suggest_splits",
    "varlen_plan", "varlen_workspace", "varlen_suggest_splits", "schedule_size", "schedule_plan", "sched_plan",
    "window_plan", "window_workspace", "window_suggest_splits", "tree_plan", "tree_workspace", "tree_suggest_splits",
)


def structs(case):
    """The structs of a case: (params, varlen_q or None, fp8 or None, tree or None)."""
    c = dict(DEFAULTS, **case)
    B, H, Hk, Nq, D, cap, page = c["B"], c["H"], c["Hk"], c["Nq"], c["D"], c["cap"], c["page"]
    p = _lib.TfaKvcacheParams()
    p.q = p.out = p.lse = p.k_cache = p.v_cache = p.cache_seqlens = ADDR
    p.B, p.H, p.Hk, p.D, p.capacity = B, H, Hk, D, cap
    vq = None
    if c["vq"] is not None:         # q (total_q, H, D), out (H, total_q, D): strides {ignored, head, row}
        mq, tq = c["vq"]
        vq = _lib.TfaKvcacheVarlenQ()
        vq.cu_seqlens_q, vq.max_seqlen_q, vq.total_q = ADDR, mq, tq
        p.q_stride[0], p.q_stride[1], p.q_stride[2] = 0, D, H * D
        p.o_stride[0], p.o_stride[1], p.o_stride[2] = 0, tq * D, D
    else:                           # q (B, Nq, H, D), out (B, H, Nq, D)
        p.Nq = Nq
        p.q_stride[0], p.q_stride[1], p.q_stride[2] = Nq * H * D, D, H * D
        p.o_stride[0], p.o_stride[1], p.o_stride[2] = H * Nq * D, Nq * D, D
    rows = page if page else cap
    for name in ("k_stride", "v_stride"):
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = rows * Hk * D, D, Hk * D
    if page:
        p.block_table, p.block_table_stride, p.page_size, p.num_pages = ADDR, cap // page, page, B * (cap // page)
    p.softmax_scale, p.is_causal, p.dtype = 0.125, c["causal"], c["dtype"]
    q8 = None
    if c["fp8"]:
        q8 = _lib.TfaKvcacheFp8()
        q8.format = _lib.TFA_KV_E4M3
        q8.k_descale = q8.v_descale = ADDR
        q8.k_descale_stride[0] = q8.v_descale_stride[0] = Hk
        q8.k_descale_stride[1] = q8.v_descale_stride[1] = 1
    tree = None
    if c["tree"]:                   # 1: present, 2: misaligned, 0: the tree entry points get NULL
        tree = _lib.TfaKvcacheTree()
        tree.mask = ADDR + (4 if c["tree"] == 2 else 0)
        tree.batch_stride, tree.row_stride = (0 if vq is not None else Nq), 1
    for m in c["mut"]:
        mutate(m, p, vq, q8, tree, c)
    return p, vq, q8, tree


def mutate(m, p, vq, q8, tree, c):
    """One named edit: "null:<pointer>", "misalign:<pointer>", or a refusal (or fallback) of its own."""
    kind, _, name = m.partition(":")
    owner = {"cu_seqlens_q": vq, "tree_mask": tree, "k_descale": q8, "v_descale": q8}.get(name, p)
    field = "mask" if name == "tree_mask" else name
    if kind == "null":
        setattr(owner, field, None)
    elif kind == "misalign":
        setattr(owner, field, ADDR + 2)
    elif m == "reserved":
        p.reserved_ = 1
    elif m == "reserved2":
        p.reserved2_ = 1
    elif m == "vq_reserved":
        vq.reserved_[1] = 1
    elif m == "q8_reserved":
        q8.reserved_ = 1
    elif m == "q8_format":
        q8.format = 7
    elif m == "group_past_2gib":    # a q head stride that puts a packed group's extent past 2 GiB: (G - 1) * stride * 2 bytes
        p.q_stride[1] = 1 << 29
    elif m == "out_noncontig":
        p.o_stride[2] = 2 * c["D"]
    elif m == "out_head_stride":
        p.o_stride[1] += 8
    elif m == "out_batch_stride":
        p.o_stride[0] += 8
    elif m == "k_new":
        p.k_new = p.v_new = ADDR
        p.n_new = 2
        for nm in ("knew_stride", "vnew_stride"):
            arr = getattr(p, nm)
            arr[0], arr[1], arr[2] = 2 * c["Hk"] * c["D"], c["D"], c["Hk"] * c["D"]
    elif m == "k_new_only":
        p.k_new = ADDR
        p.n_new = 2
    elif m == "tree_row_stride":
        tree.row_stride = -1
    elif m == "tree_batch_stride":
        tree.batch_stride = -1
    elif m == "bt_stride":
        p.block_table_stride = 1
    elif m == "k_row_stride":
        p.k_stride[2] = c["D"] - 8
    elif m == "scale":
        p.softmax_scale = 0.0
    else:
        raise ValueError(m)


def answers(L, case):
    """What every entry point of ENTRY_POINTS answers to the case."""
    c = dict(DEFAULTS, **case)
    p, vq, q8, tree = structs(case)
    r = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    P, V, Q, T = r(p), r(vq), r(q8), r(tree)
    s, pk, left, sched, causal = c["splits"], c["pack"], c["left"], c["sched"], c["causal"]

    def plan(fn, *args):
        g, b, l = C.c_int(), C.c_int(), C.c_int()
        return [fn(*args, C.byref(g), C.byref(b), C.byref(l)), g.value, b.value, l.value]

    return [
        plan(L.tfa_fwd_kvcache_plan, P, s), L.tfa_fwd_kvcache_workspace(P, s), L.tfa_fwd_kvcache_suggest_splits(P),
        plan(L.tfa_fwd_kvcache_fp8_plan, P, Q, s), L.tfa_fwd_kvcache_fp8_workspace(P, Q, s),
        plan(L.tfa_fwd_kvcache_pack_plan, P, Q, pk, s), L.tfa_fwd_kvcache_pack_workspace(P, Q, pk, s), L.tfa_fwd_kvcache_pack_suggest_splits(P, pk),
        plan(L.tfa_fwd_kvcache_varlen_plan, P, V, Q, pk, s), L.tfa_fwd_kvcache_varlen_workspace(P, V, Q, pk, s), L.tfa_fwd_kvcache_varlen_suggest_splits(P, V, pk),
        L.tfa_kvcache_varlen_schedule_size(P, V, pk, causal), plan(L.tfa_kvcache_varlen_schedule_plan, P, V, pk, causal),
        plan(L.tfa_fwd_kvcache_varlen_sched_plan, P, V, Q, pk, s),
        plan(L.tfa_fwd_kvcache_window_plan, P, V, Q, pk, left, s, sched), L.tfa_fwd_kvcache_window_workspace(P, V, Q, pk, left, s),
        L.tfa_fwd_kvcache_window_suggest_splits(P, V, pk, left),
        plan(L.tfa_fwd_kvcache_tree_plan, P, V, Q, pk, T, s, sched), L.tfa_fwd_kvcache_tree_workspace(P, V, Q, pk, T, s), L.tfa_fwd_kvcache_tree_suggest_splits(P, V, pk, T),
    ]


def grid():
    """The cases — a few hundred, no cross product: every (head dim, GQA group, row count) of both layouts with the other dimensions drawn at random (seeded), the
    split suggestion where it says more than 1, then the refusals one by one."""
    rnd = random.Random(20240611)
    dims = dict(cappage=[(n, pg) for n in (1024, 16384, 65536) for pg in (0, 128)], splits=[1, 3, 64, 1000], pack=[0, 1, 2, 7], causal=[1, 0], fp8=[0, 1],
                left=[-1, 0, 63, 1023, 1 << 30], sched=[0, 1], tree=[0, 1, 2], dtype=[_lib.TFA_BF16, _lib.TFA_F16])
    cases = []
    for D in (64, 72, 128, 256):
        for H, Hk in ((8, 8), (8, 2), (8, 1), (256, 1)):
            for rows in (dict(Nq=1), dict(Nq=5), dict(Nq=33), dict(Nq=130), dict(vq=[1, 3]), dict(vq=[5, 9]), dict(vq=[130, 200]), dict(vq=[5, 3])):
                c = dict(rows, D=D, H=H, Hk=Hk, **{k: rnd.choice(v) for k, v in dims.items()})
                c["cap"], c["page"] = c.pop("cappage")
                cases.append(c)
    # the split suggestion where it says more than 1: few workgroups over a long cache
    for B in (1, 8, 40):
        for H, Hk in ((8, 8), (32, 8)):
            for cap in (4096, 65536):
                cases.append(dict(B=B, H=H, Hk=Hk, Nq=1, cap=cap, pack=rnd.choice((0, 1, 2)), left=1023, tree=1))
                cases.append(dict(B=B, H=H, Hk=Hk, Nq=5, cap=cap, pack=rnd.choice((0, 1, 2)), causal=0))
                cases.append(dict(B=B, H=H, Hk=Hk, vq=[5, 9], cap=cap, pack=rnd.choice((0, 1, 2)), left=63, tree=1))
    # the refusals (and the packing's fallback) on the 4-D, the packed-q and the scheduled layout, each call with a window and a tree at hand
    for lay in (dict(), dict(vq=[5, 9]), dict(vq=[5, 9], sched=1)):
        full = dict(lay, left=63, tree=1, page=128, fp8=1, splits=3)          # every pointer argument is in use
        for ptr in POINTERS:
            if ptr != "cu_seqlens_q" or "vq" in lay:
                cases += [dict(full, mut=["null:" + ptr]), dict(full, mut=["misalign:" + ptr])]
        cases += [dict(full, mut=[m]) for m in ("q8_reserved", "q8_format", "bt_stride") + (("vq_reserved",) if "vq" in lay else ())]
        for splits in (1, 3):
            base = dict(lay, left=63, tree=1, splits=splits, pack=1)
            cases += [dict(base, mut=[m]) for m in ("reserved", "reserved2", "group_past_2gib", "out_noncontig", "out_head_stride", "out_batch_stride", "k_new",
                                                     "k_new_only", "tree_row_stride", "tree_batch_stride", "k_row_stride", "scale")]
            cases.append(dict(base, pack=2, mut=["group_past_2gib"]))        # (the unpacked plan a group past 2 GiB falls back to)
        base = dict(lay, left=63, tree=1)
        cases += [dict(base, Nq=1, mut=["group_past_2gib"]), dict(base, H=8, Hk=3), dict(base, H=8, Hk=3, Nq=1), dict(base, causal=0), dict(base, left=-2),
                  dict(base, tree=2), dict(base, tree=0)]
        for bad in (dict(B=0), dict(H=0), dict(Hk=0), dict(Nq=0), dict(cap=0), dict(splits=0), dict(D=0), dict(D=136), dict(dtype=_lib.TFA_F32), dict(vq=[0, 9]),
                    dict(vq=[5, 0]), dict(page=96), dict(cap=1000, page=128)):
            if "vq" not in bad or "vq" in lay:
                cases.append(dict(base, **bad))
    return cases


def main():
    L = _lib.lib()
    rows = [{"case": c, "answers": answers(L, c)} for c in grid()]
    with open(OUT, "w") as f:
        f.write('{"entry_points": ' + json.dumps(list(ENTRY_POINTS)) + ', "cases": [\n')
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n]}\n")
    print(f"{OUT}: {len(rows)} cases x {len(ENTRY_POINTS)} entry points = {len(rows) * len(ENTRY_POINTS)} rows, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
