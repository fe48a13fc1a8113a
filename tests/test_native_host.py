"""The layer the Python wrappers share (efficientconformer_amd/_native.py) and the encoder's stream plan, host side: no GPU and no libeffconf.so -
``Handle`` drives a fake library that records its calls."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

from efficientconformer_amd import ConformerEncoder, _lib, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = "EFFCONF_POISON_WORKSPACE"


# ---------------------------------------------------------------- workspace()
def test_workspace_is_plain_uint8_without_the_variable(monkeypatch):
    monkeypatch.delenv(POISON, raising=False)
    for n in (0, 1, 4097):
        ws = _native.workspace(n, "cpu")
        assert ws.dtype == torch.uint8 and ws.shape == (n,) and ws.device.type == "cpu" and ws.is_contiguous()


@pytest.mark.parametrize("fill", ["0", "127", "255"])
def test_workspace_is_filled_with_the_byte_read_at_call_time(monkeypatch, fill):
    monkeypatch.setenv(POISON, fill)
    ws = _native.workspace(4097, torch.device("cpu"))
    assert ws.dtype == torch.uint8 and ws.shape == (4097,)
    assert bool((ws == int(fill)).all())
    monkeypatch.setenv(POISON, "3")                    # per call, not at import: tests set it per test
    assert bool((_native.workspace(16, "cpu") == 3).all())


def test_the_poison_variable_lives_in_native_only():
    holders = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(ROOT, "efficientconformer_amd", "*.py")))
               if POISON in open(p, encoding="utf-8").read()]
    assert holders == ["_native.py"]


# ---------------------------------------------------------------- Handle
class FakeLib:
    """Records (entry, arguments) of every call; a tensor upload is recorded as (key, values, shape array, ndim)."""

    def __init__(self, family="lm"):
        self.calls, self.next, self.fail, self.error = [], 1000, {}, b"fake reason"
        for what in ("create", "destroy", "load_tensor", "finalize"):
            setattr(self, "effconf_%s_%s" % (family, what), getattr(self, "_" + what))

    def names(self):
        return [c[0] for c in self.calls]

    def effconf_last_error(self):
        return self.error

    def _create(self, cfg):
        self.calls.append(("create", cfg))
        if self.fail.get("create"):
            return None
        self.next += 1
        return self.next

    def _destroy(self, h):
        self.calls.append(("destroy", h))

    def _load_tensor(self, h, key, data, shape, ndim):
        shape = list(shape)
        n = int(np.prod(shape[:ndim])) if ndim else 1
        values = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_float)), shape=(n,)).copy()      # what a C reader of contiguous fp32 sees
        self.calls.append(("load_tensor", h, key, values, shape, ndim))
        return 7 if self.fail.get("load_tensor") == key else 0

    def _finalize(self, h):
        self.calls.append(("finalize", h))
        return 9 if self.fail.get("finalize") else 0


def _cfg():
    return _lib.EcLmConfig(8, 16, 1)


def test_handle_rebuild_call_order_and_tensor_upload():
    lib = FakeLib()
    h = _native.Handle("lm", lib)
    assert h.ptr is None
    base = torch.arange(12, dtype=torch.int32).reshape(3, 4)
    tensors = [("a.weight", base.t()),                                   # int32, not contiguous: goes up as contiguous fp32 (4, 3)
               ("b.scalar", torch.tensor(2.5, dtype=torch.float64)),     # 0-d: goes up as one element, a shape array of length 1
               ("c.bias", torch.tensor([1.0, -2.0], requires_grad=True))]
    seen = []

    def before_load(ptr):
        seen.append(ptr)
        lib.calls.append(("before_load", ptr))

    h.rebuild(_cfg(), tensors, before_load)
    assert h.ptr == 1001 and seen == [1001]
    assert lib.names() == ["create", "before_load", "load_tensor", "load_tensor", "load_tensor", "finalize"]
    loads = [c for c in lib.calls if c[0] == "load_tensor"]
    assert [c[2] for c in loads] == [b"a.weight", b"b.scalar", b"c.bias"] and all(c[1] == 1001 for c in loads)
    assert loads[0][4] == [4, 3] and loads[0][5] == 2
    assert loads[0][3].dtype == np.float32 and loads[0][3].tolist() == base.t().contiguous().reshape(-1).float().tolist()
    assert loads[1][4] == [1] and loads[1][5] == 1 and loads[1][3].tolist() == [2.5]
    assert loads[2][4] == [2] and loads[2][5] == 1 and loads[2][3].tolist() == [1.0, -2.0]
    assert lib.calls[-1] == ("finalize", 1001)


def test_handle_second_rebuild_destroys_the_first_handle_before_it_creates():
    lib = FakeLib("rnnt")
    h = _native.Handle("rnnt", lib)
    h.rebuild(_cfg(), [])
    h.rebuild(_cfg(), [("w", torch.zeros(2))])
    assert lib.names() == ["create", "finalize", "destroy", "create", "load_tensor", "finalize"]
    assert lib.calls[2] == ("destroy", 1001) and h.ptr == 1002


def test_handle_errors_name_the_entry_the_key_and_the_librarys_reason():
    lib = FakeLib()
    lib.fail["create"] = True
    h = _native.Handle("lm", lib)
    with pytest.raises(_lib.EffconfError, match=r"^effconf_lm_create: fake reason$"):
        h.rebuild(_cfg(), [])
    assert h.ptr is None
    lib.fail = {"load_tensor": b"k2"}
    with pytest.raises(_lib.EffconfError, match=r"^lm_load_tensor\(k2\) failed \(rc=7\): fake reason$"):
        h.rebuild(_cfg(), [("k1", torch.zeros(1)), ("k2", torch.zeros(1)), ("k3", torch.zeros(1))])
    assert lib.names()[-2:] == ["load_tensor", "load_tensor"]            # k3 never went up, nothing was finalized
    failed = h.ptr
    lib.fail = {"finalize": True}
    n = len(lib.calls)
    with pytest.raises(_lib.EffconfError, match=r"^lm_finalize failed \(rc=9\): fake reason$"):
        h.rebuild(_cfg(), [])
    assert lib.calls[n] == ("destroy", failed)                           # the handle of the failed rebuild is destroyed by the next one
    enc = FakeLib("encoder")                                             # the encoder's texts carry no family name
    enc.fail = {"load_tensor": b"fc.weight"}
    with pytest.raises(_lib.EffconfError, match=r"^load_tensor\(fc.weight\) failed \(rc=7\): fake reason$"):
        _native.Handle("encoder", enc).rebuild(_cfg(), [("fc.weight", torch.zeros(1))])
    enc.fail = {"finalize": True}
    with pytest.raises(_lib.EffconfError, match=r"^finalize failed \(rc=9\): fake reason$"):
        _native.Handle("encoder", enc).rebuild(_cfg(), [])


def test_handle_close_is_idempotent():
    lib = FakeLib()
    h = _native.Handle("lm", lib)
    h.close()                                          # nothing to destroy yet
    assert lib.calls == []
    h.rebuild(_cfg(), [])
    h.close()
    h.close()
    assert lib.names().count("destroy") == 1 and h.ptr is None
    h.__del__()
    assert lib.names().count("destroy") == 1


def test_handle_del_without_a_library_does_nothing(monkeypatch):
    lib = FakeLib()
    h = _native.Handle("lm", lib)
    h.rebuild(_cfg(), [])
    h._lib = None                                      # the library reference is gone ...
    monkeypatch.setattr(_lib, "_lib", None)            # ... and libeffconf.so is not (or no longer) loaded
    h.__del__()
    assert "destroy" not in lib.names() and h.ptr == 1001
    h.ptr = None                                       # nothing left for the real __del__ at collection


# ---------------------------------------------------------------- lengths()
def test_lengths_default_and_conversion():
    full = _native.lengths(None, 3, 41, "cpu")
    assert full.dtype == torch.int64 and full.shape == (3,) and full.tolist() == [41, 41, 41]
    src = torch.tensor([[5, 0], [7, 0], [9, 0]], dtype=torch.int32)[:, 0]
    assert not src.is_contiguous()
    got = _native.lengths(src, 3, 41, torch.device("cpu"))
    assert got.dtype == torch.int64 and got.is_contiguous() and got.device.type == "cpu" and got.tolist() == [5, 7, 9]
    ready = torch.tensor([4, 2], dtype=torch.int64)
    assert _native.lengths(ready, 2, 9, "cpu") is ready                  # nothing to convert: the caller's own tensor (the encoder's length memo needs that)


# ---------------------------------------------------------------- sized()
class _Reason:
    @staticmethod
    def effconf_last_error():
        return b"why not"


def test_sized_returns_the_size_or_raises_the_six_texts():
    assert _native.sized(_Reason, "effconf_lm", 4096, n=1, U=2) == 4096
    cases = [
        ("effconf_ctc_beam", dict(batch=3, T=17, vocab=2000, beam=4),
         "effconf_ctc_beam_workspace_bytes rejected (batch 3, T 17, vocab 2000, beam 4): why not"),
        ("effconf_ctc_align", dict(batch=2, T=9, vocab=1, U=5),
         "effconf_ctc_align_workspace_bytes rejected (batch 2, T 9, vocab 1, U 5): why not"),
        ("effconf_rnnt_beam", dict(batch=1, T=0, beam=4, max_expansions=64, max_tokens=16),
         "effconf_rnnt_beam_workspace_bytes rejected (batch 1, T 0, beam 4, max_expansions 64, max_tokens 16): why not"),
        ("effconf_rnnt_lattice", dict(batch=-1, T=3, U=2), "effconf_rnnt_lattice_workspace_bytes rejected (batch -1, T 3, U 2): why not"),
        ("effconf_rnnt_align", dict(batch=4, T=3, U=70000), "effconf_rnnt_align_workspace_bytes rejected (batch 4, T 3, U 70000): why not"),
        ("effconf_lm", dict(n=64, U=-2), "effconf_lm_workspace_bytes rejected (n 64, U -2): why not"),
    ]
    for entry, args, text in cases:
        with pytest.raises(_lib.EffconfError) as e:
            _native.sized(_Reason, entry, 0, **args)
        assert str(e.value) == text


def test_require_hip_refuses_a_host_tensor():
    with pytest.raises(RuntimeError, match=r"^efficientconformer_amd runs on a HIP device only \(no CPU fallback\)$"):
        _native.require_hip(torch.zeros(1))


# ---------------------------------------------------------------- the stream plan
@pytest.mark.parametrize("args, plan", [
    ((3, None, True), [(1, 1, False), (2, 2, False), (0, 0, True)]),
    ((4, 2, True), [(1, 1, False), (3, 1, False), (0, 0, True), (2, 0, True)]),
    ((3, None, False), [(0, 0, False), (1, 1, False), (2, 2, False)]),
    ((4, 2, False), [(0, 0, False), (1, 1, False), (2, 0, False), (3, 1, False)]),
    ((3, 8, True), [(1, 1, False), (2, 2, False), (0, 0, True)]),        # more streams than ranges: one per range
    ((3, 1, True), [(0, 0, True), (1, 0, True), (2, 0, True)]),          # one stream: everything on the caller's, in order
    ((1, None, True), [(0, 0, True)]),
    ((1, 3, False), [(0, 0, False)]),
])
def test_stream_plan_against_a_hand_written_table(args, plan):
    assert ConformerEncoder.stream_plan(*args) == plan
