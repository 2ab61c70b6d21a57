"""QuipQuantizer.quantize_model and the LDLQ panel route without a GPU: what is refused (by name, before the model is
touched), the calibration data forms and batching on CPU tensors, the QUIP_LDLQ_FUSED switch, the C entry's argument
checks, and the panel arithmetic of quant.LDLQ_panels against stepwise LDLQ with the float64 brute force as the search."""
import ctypes
import types

import numpy as np
import pytest
import torch

from quip_for_all_amd import quant
from quip_for_all_amd.quantizer import QuipQuantizer, calibration_batches, calibration_samples

from tests import ldlq_cases as C

IDS = [[(7 * i + 3 * j) % 50 for j in range(16)] for i in range(6)]


class _Untouchable:
    """a model that fails the test as soon as anything is read from it"""

    def __getattr__(self, name):
        if name == "hf_device_map":
            raise AttributeError(name)
        raise AssertionError(f"model.{name} was touched before the refusal")


# ---- refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dataset", ["", "wikitext2", "c4"])
def test_dataset_names_are_refused_by_name(dataset):
    q = QuipQuantizer(codebook="E8P12", dataset=dataset, ft_epochs=0)
    for model in (None, _Untouchable()):
        with pytest.raises(NotImplementedError) as e:
            q.quantize_model(model, None)
        msg = str(e.value)
        assert "dataset loaders" in msg and "not part of this build" in msg
        assert "list of strings" in msg and "token-id sequences" in msg and "dicts with `input_ids`" in msg


def test_default_ft_epochs_is_refused_and_says_how():
    q = QuipQuantizer(codebook="E8P12", dataset=IDS)                # ft_epochs defaults to 5
    for model in (None, _Untouchable()):
        with pytest.raises(NotImplementedError, match="pass ft_epochs=0"):
            q.quantize_model(model, None)


def test_merge_suv_is_refused():
    q = QuipQuantizer(codebook="E8P12", dataset=IDS, ft_epochs=0, merge_suv=True)
    for model in (None, _Untouchable()):
        with pytest.raises(NotImplementedError, match="merge_suv"):
            q.quantize_model(model, None)


def test_dispatched_model_is_refused():
    q = QuipQuantizer(codebook="E8P12", dataset=IDS, ft_epochs=0)
    model = types.SimpleNamespace(hf_device_map={"": 0})
    with pytest.raises(NotImplementedError, match="hf_device_map"):
        q.quantize_model(model, None)


def test_refusal_order_dataset_first():
    """the constructor's defaults (dataset "", ft_epochs 5): the dataset is named first"""
    with pytest.raises(NotImplementedError, match="dataset loaders"):
        QuipQuantizer(codebook="E8P12").quantize_model(None, None)


# ---- calibration data ------------------------------------------------------------------------------------------------------
class _Tok:
    """a trivial tokenizer: one id per whitespace-separated number"""

    def __call__(self, text):
        return {"input_ids": [int(w) for w in text.split()]}


def test_three_dataset_forms_give_the_same_samples():
    lists = calibration_samples(IDS, None, 16)
    tensors = calibration_samples([torch.tensor(r) for r in IDS], None, 16)
    arrays = calibration_samples([np.asarray(r)[None] for r in IDS], None, 16)           # (1, L) is flattened
    dicts = calibration_samples([{"input_ids": torch.tensor(r)} for r in IDS], None, 16)
    strings = calibration_samples([" ".join(map(str, r)) for r in IDS], _Tok(), 16)
    for form in (lists, tensors, arrays, dicts, strings):
        assert len(form) == len(IDS)
        for s, r in zip(form, IDS):
            assert s["input_ids"].dtype == torch.long and tuple(s["input_ids"].shape) == (1, 16)
            assert s["input_ids"][0].tolist() == r and s["attention_mask"].tolist() == [[1] * 16]
            assert s["input_ids"].device.type == "cpu"


def test_strings_are_packed_and_sequences_are_cut():
    flat = [t for r in IDS for t in r]                                  # 96 ids
    texts = [" ".join(map(str, flat[:5])), " ".join(map(str, flat[5:50])), " ".join(map(str, flat[50:]))]
    packed = calibration_samples(texts, _Tok(), 40)                      # 96 = 2 x 40 + a dropped rest of 16
    assert [s["input_ids"][0].tolist() for s in packed] == [flat[:40], flat[40:80]]
    short = calibration_samples(texts[:1], _Tok(), 40)                   # less than one sample: kept as it is
    assert short[0]["input_ids"][0].tolist() == flat[:5]
    cut = calibration_samples(IDS, None, 10)
    assert all(s["input_ids"][0].tolist() == r[:10] for s, r in zip(cut, IDS))
    masked = calibration_samples([{"input_ids": IDS[0], "attention_mask": [1] * 12 + [0] * 4}], None, 14)
    assert masked[0]["attention_mask"].tolist() == [[1] * 12 + [0] * 2]


def test_bad_datasets_raise():
    with pytest.raises(ValueError, match="empty"):
        calibration_samples([], None, 16)
    with pytest.raises(ValueError, match="tokenizer"):
        calibration_samples(["1 2 3"], None, 16)
    with pytest.raises(ValueError, match="input_ids"):
        calibration_samples([{"ids": [1, 2]}], None, 16)
    with pytest.raises(ValueError, match="mixes"):
        calibration_samples([[1, 2], "3 4"], _Tok(), 16)
    with pytest.raises(ValueError, match="differ in length"):
        calibration_samples([{"input_ids": [1, 2, 3], "attention_mask": [1, 1]}], None, 16)


def test_batching():
    samples = calibration_samples(IDS, None, 16)
    b = calibration_batches(samples, nsamples=5, batch_size=2)          # 5 of 6 samples: 2 + 2 + 1
    assert [tuple(x["input_ids"].shape) for x in b] == [(2, 16), (2, 16), (1, 16)]
    assert torch.cat([x["input_ids"] for x in b]).tolist() == IDS[:5]
    assert all(x["attention_mask"].shape == x["input_ids"].shape and x["input_ids"].dtype == torch.long for x in b)
    assert len(calibration_batches(samples, nsamples=4096, batch_size=4)) == 2           # fewer samples than nsamples
    ragged = calibration_samples([IDS[0], IDS[1][:9]], None, 16)
    with pytest.raises(ValueError, match="differ in length"):
        calibration_batches(ragged, 2, 2)
    assert len(calibration_batches(ragged, 2, 1)) == 2
    with pytest.raises(ValueError):
        calibration_batches(samples, 4, 0)


# ---- the switch --------------------------------------------------------------------------------------------------------------
def test_ldlq_fused_switch_parses(monkeypatch):
    assert quant.parse_ldlq_fused(None) is True and quant.parse_ldlq_fused("") is True
    assert quant.parse_ldlq_fused("0") is False and quant.parse_ldlq_fused(" 0 ") is False
    assert quant.parse_ldlq_fused("1") is True and quant.parse_ldlq_fused("on") is True
    assert quant.parse_ldlq_fused(None, default=False) is False
    monkeypatch.setattr(quant, "_LDLQ_FUSED", None)
    monkeypatch.setenv("QUIP_LDLQ_FUSED", "0")
    assert quant.ldlq_fused_enabled() is False
    monkeypatch.setenv("QUIP_LDLQ_FUSED", "1")
    assert quant.ldlq_fused_enabled() is False                            # read once per process
    monkeypatch.setattr(quant, "_LDLQ_FUSED", None)
    assert quant.ldlq_fused_enabled() is True


def test_route_is_stepwise_off_the_gpu_and_for_other_codebooks():
    W = torch.zeros(4, 16)
    assert quant.ldlq_route(W, C.OracleCodebook()) == "stepwise"        # a CPU tensor
    assert quant.ldlq_route(W.double(), C.OracleCodebook()) == "stepwise"
    assert quant.panel_bounds(688, 8, 128) == [(560, 688), (432, 560), (304, 432), (176, 304), (48, 176), (0, 48)]
    assert quant.panel_bounds(8, 8, 128) == [(0, 8)] and quant.panel_bounds(64, 8, 16)[-1] == (0, 16)


# ---- the C entry: every refusal comes before a launch -------------------------------------------------------------------
def test_c_entry_checks_its_arguments():
    from quip_for_all_amd import capi
    L = capi.lib()
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 63) & ~63
    f = L.quip_ldlq_panel_f32
    assert f(a, a, a, None, 0, 128, a, a, a, None) == 0            # m == 0: ok, no launch
    assert f(a, a, a, None, -1, 128, a, a, a, None) == -2
    assert f(a, a, a, None, 4, 12, a, a, a, None) == -2            # c % 8
    assert f(a, a, a, None, 4, 0, a, a, a, None) == -2
    assert f(a, a, a, None, 4, 136, a, a, a, None) == -5           # c > 128
    for hole in range(3):
        args = [a, a, a]
        args[hole] = None
        assert f(*args, None, 4, 8, a, a, a, None) == -1
    assert f(a, a, a, None, 4, 8, None, a, a, None) == -1 and f(a, a, a, None, 4, 8, a, None, a, None) == -1
    assert f(a, a, a, None, 4, 8, a, a, None, None) == -1
    assert f(a + 4, a, a, None, 4, 8, a, a, a, None) == -3 and f(a, a, a, a + 4, 4, 8, a, a, a, None) == -3
    assert f(a, a, a, None, 4, 8, a, a, a + 4, None) == -3         # idx: 8-byte aligned


def test_op_fake_shapes():
    t = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")   # noqa: E731
    hat, idx = torch.ops.quip_lib.ldlq_panel(t(40, 48), t(40, 48), t(48, 48), None, t(256, dtype=torch.int64))
    assert (tuple(hat.shape), hat.dtype, tuple(idx.shape), idx.dtype) == ((40, 48), torch.float32, (40, 6), torch.int64)
    hat, idx = torch.ops.quip_lib.ldlq_panel(t(3, 8), t(3, 8), t(8, 8), t(1, 8, 8), t(256, dtype=torch.int64))
    assert tuple(idx.shape) == (3, 1)


# ---- the panel arithmetic ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case384():
    W, H = C.make_case(40, 384)
    Wt, Ht = torch.from_numpy(W).double(), torch.from_numpy(H).double()
    return Wt, Ht, torch.linalg.cholesky(Ht)


@pytest.mark.parametrize("iters", [0, 1])
def test_panel_recursion_reproduces_stepwise_ldlq(case384, iters):
    """A torch model of the recursion of ldlq_panel (tests/ldlq_cases.panel_model), driven by quant.LDLQ_panels exactly as
    the kernel is, against quant.LDLQ_stepwise -- both in float64 with the brute force as the search, so that they differ
    by float64 rounding of the targets only: the indices are equal, or, where a tie resolved differently, of equal
    distance to the stepwise target."""
    W, H, L = case384
    cb = C.OracleCodebook()
    hat_s, q_s = quant.LDLQ_stepwise(W.clone(), H.clone(), L.clone(), cb, iters)
    hat_p, q_p = quant.LDLQ_panels(W.clone(), H.clone(), L.clone(), cb, iters, panel_fn=C.panel_model)
    diff = (q_s != q_p).nonzero()
    if len(diff):
        row, col = (int(v) for v in diff[diff[:, 1].argmax()])          # the first group rounded (rightmost) that differs
        assert iters == 0, "ties are settled in the main pass"
        Lb = quant.block_LDL(L.clone(), 8)
        lo, hi = 8 * col, 8 * col + 8
        t = W[row, lo:hi] + (W[row, hi:] - hat_s[row, hi:]) @ Lb[hi:, lo:hi]
        d_s, d_p = (t - hat_s[row, lo:hi]).norm().item(), (t - hat_p[row, lo:hi]).norm().item()
        assert abs(d_s - d_p) <= 1e-12, (row, col, d_s, d_p)
        keep = torch.ones(W.shape[0], dtype=torch.bool)
        keep[diff[:, 0].unique()] = False                                  # rows without a tie must agree entirely
        assert torch.equal(q_s[keep], q_p[keep])
        assert (~keep).sum() <= 1
    else:
        assert torch.equal(hat_s, hat_p)


def test_stepwise_fp32_meets_the_float64_step_check(case384):
    """what tests/test_gpu_ldlq_panel.py asks of the kernel, met by the repository's own fp32 stepwise loop on the CPU"""
    W, H, L = case384
    hat, _ = quant.LDLQ_stepwise(W.float(), H.float(), L.float(), C.OracleCodebook(), 0)
    Lb = C.O.block_ldl(L.numpy(), 8)
    over, steps, _ = C.check_ldlq_steps(W.numpy(), Lb, hat.numpy())
    assert (over, steps) == (0, 1920)
