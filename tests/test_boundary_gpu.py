"""The C boundary as an integrator calls it: the flat entry points tfa_fwd_bhnd / tfa_fwd_bhnd_f32out (what INTEGRATION.md tells a host to call) run on the GPU —
through ctypes on the current stream, and from a host program without Python or torch (tests/c_host/tfa_host.c, built next to the library by csrc/Makefile).

Every 16-bit case (fwd_ref.BHND_CASES: the second 256-row block, a head dim below the kernel's width, the 256-wide kernel) asserts
  * out and lse are bit for bit those of ops.flash_attn_fwd on the same tensors (the _f32out call: out_f32=True), and
  * they sit within the per-element bounds of tests/fwd_ref.py — out_ratio <= 1 for the 16-bit and the fp32 out, lse_ratio <= 1 against lse_bound, no NaN, and
    lse = +inf / out = 0 exactly on the rows that see no key — against fp64, never against another run of the kernels.
tests/test_fwd_bounds_cpu.py proves on the CPU that the correct algorithm fits these bounds on these cases.  The fp32 case (TFA_F32 inputs, lse = NULL) is held to
tests/test_f32_gpu.py's bar, 2e-5 against fp64, with a sentinel behind out.  max(|d| / bound) is printed before it is asserted."""
import ctypes as C
import functools
import os
import struct
import subprocess

import pytest
import torch

import fwd_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiny-flash-attention_amd", "lib", "tfa_host")
HOST_CASES = [("bhnd-bf16-b2h4-d128-c-320", False), ("bhnd-fp16-b1h2-d256-c-200", True)]      # (case, through tfa_fwd_bhnd_f32out): one child process each


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from tiny_flash_attention_amd import _lib

    _lib.lib()
    return _lib


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """The case's tensors and the fp64 reference with its bounds: computed once on the CPU, shared by the ctypes and the C-host test, never modified."""
    t = R.build(R.BOUNDARY_BY_ID[case_id])
    return t, R.reference(t)[None]


def flat_call(lib, t, dev, f32out):
    """tfa_fwd_bhnd / tfa_fwd_bhnd_f32out through ctypes on the current stream: (out, lse) on the device."""
    c = t["case"]
    q, k, v = (t[n].to(dev).contiguous() for n in ("q", "k", "v"))
    out = torch.empty(q.shape, dtype=torch.float32 if f32out else q.dtype, device=dev)
    lse = torch.empty(q.shape[:3], dtype=torch.float32, device=dev)
    fn = lib.lib().tfa_fwd_bhnd_f32out if f32out else lib.lib().tfa_fwd_bhnd
    with torch.cuda.device(dev):
        lib.check(fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), c["B"], c["H"], c["Nq"], c["D"], t["sc"], int(c["causal"]),
                     lib.TFA_BF16 if q.dtype == torch.bfloat16 else lib.TFA_F16, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out, lse


def public_call(t, dev, f32out):
    from tiny_flash_attention_amd import ops

    c = t["case"]
    out, lse = ops.flash_attn_fwd(t["q"].to(dev), t["k"].to(dev), t["v"].to(dev), c["causal"], t["sc"], out_f32=f32out)
    torch.cuda.synchronize()
    return out, lse


def hold_to_bounds(what, t, ref, out, lse, f32out):
    """out (B,H,N,D) and lse (B,H,N) on the CPU against the fp64 definition: the per-element bounds of tests/fwd_ref.py, no element exempt."""
    o64, l64, A, T, bound = ref
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(lse).any()), f"{what}: NaN"
    unseen = torch.isposinf(l64)
    assert torch.equal(torch.isposinf(lse), unseen), f"{what}: lse = +inf on other rows than the definition's"
    assert bool((out[unseen.unsqueeze(-1).expand_as(out)] == 0).all()), f"{what}: out != 0 on a row that sees no key"
    ro, rl = R.out_ratio(out.double(), o64, A, t["dtype"], not f32out), R.lse_ratio(lse, l64, bound)
    print(f"{what}: max(|d| / bound) {'out32' if f32out else 'out16'} {ro:.4f}  lse {rl:.4f}  (largest T {T.max().item():.1f}, rows without a key: {int(unseen.sum())})")
    assert ro <= 1.0, f"{what}: out is at {ro:.3f} of its per-element bound"
    assert rl <= 1.0, f"{what}: the LSE is at {rl:.3f} of its derived bound"


@pytest.mark.parametrize("f32out", [False, True], ids=["bhnd", "bhnd_f32out"])
@pytest.mark.parametrize("case_id", [c["id"] for c in R.BHND_CASES])
def test_flat_entry_points(lib, dev, case_id, f32out):
    t, ref = reference(case_id)
    out, lse = flat_call(lib, t, dev, f32out)
    o2, l2 = public_call(t, dev, f32out)
    assert out.dtype == o2.dtype and torch.equal(out, o2) and torch.equal(lse, l2), f"{case_id}: the flat entry point and ops.flash_attn_fwd differ in bits"
    hold_to_bounds(f"{case_id}[{'tfa_fwd_bhnd_f32out' if f32out else 'tfa_fwd_bhnd'}]", t, ref, out.cpu(), lse.cpu(), f32out)


@pytest.mark.parametrize("entry", ["tfa_fwd_bhnd", "tfa_fwd_bhnd_f32out"])
def test_flat_entry_points_fp32_inputs_without_lse(lib, dev, oracle, entry):
    """TFA_F32 q, k, v (B1 H2 N70 D72, causal) with lse = NULL: 2e-5 against fp64 (tests/test_f32_gpu.py's bar), and nothing written behind out."""
    B, H, N, D = 1, 2, 70, 72
    q, k, v = oracle.make_inputs(B, H, N, D, torch.float32, seed=11)
    sc = D ** -0.5
    n = B * H * N * D
    buf = torch.full((n + 64,), SENTINEL, dtype=torch.float32, device=dev)
    qd, kd, vd = (x.to(dev).contiguous() for x in (q, k, v))
    with torch.cuda.device(dev):
        lib.check(getattr(lib.lib(), entry)(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), buf.data_ptr(), None, B, H, N, D, sc, 1, lib.TFA_F32,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    buf = buf.cpu()
    assert bool((buf[n:] == SENTINEL).all()), "the call wrote behind out"
    exact = oracle.exact64(q, k, v, True, sc, p_round=None)
    d = (buf[:n].view(B, H, N, D).double() - exact.double()).abs().max().item()
    print(f"{entry} fp32 inputs: max|d| = {d:.3e} (bar 2e-5)")
    assert d <= 2e-5, f"max|d| = {d:.3e}"


def write_problem(path, t, f32out, want_lse=True):
    """tests/c_host/tfa_host.c's input: 12 little-endian words, then the raw bits of q, k, v."""
    c = t["case"]
    code = 1 if t["dtype"] == torch.bfloat16 else 0
    with open(path, "wb") as f:
        f.write(struct.pack("<8i", 0x48414654, code, c["B"], c["H"], c["Nq"], c["D"], int(c["causal"]), int(f32out)) + struct.pack("<f", t["sc"]) + struct.pack("<3i", int(want_lse), 0, 0))
        for n in ("q", "k", "v"):
            f.write(t[n].contiguous().view(torch.int16).numpy().tobytes())


def read_result(path, t, f32out):
    c = t["case"]
    shape = (c["B"], c["H"], c["Nq"], c["D"])
    raw = open(path, "rb").read()
    n, rows = shape[0] * shape[1] * shape[2] * shape[3], shape[0] * shape[1] * shape[2]
    osize = 4 if f32out else 2
    assert len(raw) == n * osize + rows * 4, f"{path}: {len(raw)} bytes, not out and lse of the problem"
    if f32out:
        out = torch.frombuffer(bytearray(raw[:n * 4]), dtype=torch.float32).view(shape)
    else:
        out = torch.frombuffer(bytearray(raw[:n * 2]), dtype=torch.int16).view(t["dtype"]).view(shape)
    return out, torch.frombuffer(bytearray(raw[n * osize:]), dtype=torch.float32).view(shape[:3])


@pytest.mark.parametrize("case_id,f32out", HOST_CASES, ids=[f"{c}-{'bhnd_f32out' if f else 'bhnd'}" for c, f in HOST_CASES])
def test_c_host_without_python_or_torch(dev, tmp_path, case_id, f32out):
    """The C99 host reads the problem from a file, allocates with hipMalloc, calls the flat entry point on a stream it created and writes out and lse: one child
    process per case.  The file's bits are those of ops.flash_attn_fwd in this process, and they sit within the fwd_ref bounds."""
    assert os.path.exists(HOST), f"{HOST} is missing: csrc/Makefile's `all` builds it next to the library"
    t, ref = reference(case_id)
    src, dst = str(tmp_path / "problem.bin"), str(tmp_path / "result.bin")
    write_problem(src, t, f32out)
    r = subprocess.run([HOST, "run", src, dst], timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, f"tfa_host exited {r.returncode}: {r.stderr.strip()}"
    out, lse = read_result(dst, t, f32out)
    o2, l2 = public_call(t, dev, f32out)
    hold_to_bounds(f"{case_id}[tfa_host {'f32out' if f32out else '16-bit'}]", t, ref, out, lse, f32out)
    assert torch.equal(out, o2.cpu()) and torch.equal(lse, l2.cpu()), f"{case_id}: the C host's result and ops.flash_attn_fwd differ in bits"


def test_c_host_reports_a_refusal(tmp_path):
    """A rejected argument (head dim 12) comes back as a non-zero exit with tfa_strerror's text on stderr — nothing is launched."""
    assert os.path.exists(HOST), f"{HOST} is missing: csrc/Makefile's `all` builds it next to the library"
    src, dst = str(tmp_path / "problem.bin"), str(tmp_path / "result.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<8i", 0x48414654, 1, 1, 1, 16, 12, 0, 0) + struct.pack("<f", 0.25) + struct.pack("<3i", 1, 0, 0) + bytes(3 * 16 * 12 * 2))
    r = subprocess.run([HOST, "run", src, dst], timeout=120, capture_output=True, text=True)
    assert r.returncode == 1 and "head dim" in r.stderr and not os.path.exists(dst), (r.returncode, r.stderr)
