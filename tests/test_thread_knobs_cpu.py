"""The debug knobs of include/tfa.h are state of the CALLING THREAD: "a thread that forces a variant does not change what other threads' calls run".  No GPU —
plans never launch: a thread that forces a kernel variant sees that variant's launch geometry in tfa_fwd_plan, and a thread beside it sees
tfa_get_variant() == -1 and the automatic choice's geometry, whichever of the two started first.  The threads meet through threading.Event objects, no sleeps."""
import ctypes as C
import threading
import traceback

PROBLEM = (4, 32, 32, 4096, 4096, 128, True)      # B, H, Hk, Nq, Nk, D, causal: the headline shape
WAIT = 30.0                                       # a guard against a lost event, not a timing assertion


def _params(lib):
    B, H, Hk, Nq, Nk, D, causal = PROBLEM
    p = lib.TfaFwdParams()
    p.q = p.k = p.v = p.out = 0x1000               # never dereferenced: a plan validates and sizes, nothing more
    p.lse = None
    p.B, p.H, p.Hk, p.Nq, p.Nk, p.D = B, H, Hk, Nq, Nk, D
    for name, n, h in (("q_stride", Nq, H), ("k_stride", Nk, Hk), ("v_stride", Nk, Hk), ("o_stride", Nq, H)):
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = h * n * D, n * D, D
    p.softmax_scale = 1.0
    p.is_causal = int(causal)
    p.dtype = p.out_dtype = lib.TFA_BF16
    return p


def _look(lib):
    """(tfa_get_variant(), tfa_fwd_variant, (grid, block, lds) of tfa_fwd_plan) as the calling thread sees them."""
    p = _params(lib)
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    lib.check(lib.lib().tfa_fwd_plan(C.byref(p), C.byref(g), C.byref(b), C.byref(l)))
    return lib.get_variant(), lib.lib().tfa_fwd_variant(C.byref(p)), (g.value, b.value, l.value)


def test_a_forced_variant_belongs_to_its_thread():
    from tiny_flash_attention_amd import _lib as lib

    lib.set_variant(-1)
    auto = _look(lib)
    assert auto[0] == -1 and auto[1] == lib.variant_for(*PROBLEM)
    forced = None
    for v in range(lib.num_variants()):            # a product variant whose block size differs from the automatic choice's
        if not lib.variant_available(v) or v == auto[1]:
            continue
        lib.set_variant(v)
        try:
            p = _params(lib)
            if lib.lib().tfa_fwd_plan(C.byref(p), None, None, None) == 0 and _look(lib)[2][1] != auto[2][1]:
                forced = _look(lib)
                break
        finally:
            lib.set_variant(-1)
    assert forced is not None and forced[0] == forced[1] != auto[1], "no product variant with another block size serves this problem"
    print(f"automatic: variant {auto[1]} {auto[2]};  forced: variant {forced[1]} {forced[2]}")

    seen, errors = {}, []
    started, swap, forced_there, release = (threading.Event() for _ in range(4))

    def worker():
        try:
            seen["worker beside a forcing main"] = _look(lib)
            started.set()
            assert swap.wait(WAIT)
            lib.set_variant(forced[0])                     # the roles swapped: this thread forces, the main thread must not notice
            seen["worker forcing"] = _look(lib)
            forced_there.set()
            assert release.wait(WAIT)
            seen["worker still forcing"] = _look(lib)
        except BaseException:                               # noqa: BLE001
            errors.append(traceback.format_exc())
            started.set(), forced_there.set()

    try:
        lib.set_variant(forced[0])
        th = threading.Thread(target=worker, daemon=True)
        th.start()                                          # started AFTER the main thread forced its variant
        assert started.wait(WAIT)
        seen["main forcing"] = _look(lib)
        lib.set_variant(-1)
        swap.set()
        assert forced_there.wait(WAIT)
        seen["main beside a forcing worker"] = _look(lib)
        release.set()
        th.join(WAIT)
        assert not th.is_alive()
    finally:
        release.set(), swap.set()
        lib.set_variant(-1)
    assert not errors, errors[0]
    assert seen["worker beside a forcing main"] == auto, "a thread started after another forced a variant must see -1 and the automatic choice's plan"
    assert seen["main forcing"] == forced
    assert seen["worker forcing"] == forced and seen["worker still forcing"] == forced
    assert seen["main beside a forcing worker"] == auto, "a variant forced by another thread changed the main thread's plan"
