"""quip_had_mix_batch_f16 and its route without a GPU: the header and the ABI version, the entry's refusals code
for code on host scratch pointers (aligned fake addresses: the entry checks before it launches and never dereferences,
the trick of tests/test_had_plan_host.py), the routing predicate, the switch's default."""
import ctypes
import os
import re

import pytest

from quip_for_all_amd import capi, register_lib as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "quip_had_mix_batch_f16"
OK_, NULL, SHAPE, UNSUP = 0, -1, -2, -5
_buf = (ctypes.c_char * 8192)()
P16 = ((ctypes.addressof(_buf) + 15) & ~15) + 256


def test_header_declares_the_entry_and_the_abi_version_moved():
    src = open(os.path.join(REPO, "include", "quip_mi355.h")).read()
    abi = int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1))
    assert ENTRY in src and ENTRY in capi.SIGNATURES and hasattr(capi.lib(), ENTRY)
    assert abi >= 25 and capi.lib().quip_abi_version() == abi


def _call(rows=32, n=13824, K=27, fin=None, fout=None, **fields):
    base = dict(x=P16, out=P16 + 1024, had=P16 + 2048, in_features=n if fin is None else fin,
                out_features=n if fout is None else fout, scale=1.0)
    pr = capi.HadProblem(**{**base, **fields})
    return capi.lib().quip_had_mix_batch_f16(ctypes.byref(pr), rows, n, K, 0, None)


V = P16 + 4096   # a present, aligned vector
REFUSALS = [
    (NULL, dict(x=None)), (NULL, dict(out=None)), (NULL, dict(had=None)),
    (SHAPE, dict(n=13825)),                       # K does not divide n
    (SHAPE, dict(n=27 * 768)),                    # L not a power of two
    (SHAPE, dict(fin=13832)), (SHAPE, dict(fout=0)),
    (UNSUP, dict(n=27 * 256)), (UNSUP, dict(n=8 * 2048, K=8)),            # L outside {512, 1024}
    (UNSUP, dict(n=49 * 512, K=49)), (UNSUP, dict(n=1024, K=1)),
    (UNSUP, dict(n=29 * 1024, K=29)),             # K L > 28672
    (UNSUP, dict(rows=31)),
    (UNSUP, dict(x=P16 + 2)), (UNSUP, dict(out=P16 + 1032)), (UNSUP, dict(pre_scale=V + 8)), (UNSUP, dict(residual=V + 4)),
    (UNSUP, dict(fout=13820)), (UNSUP, dict(fin=13820)),
    (UNSUP, dict(rms_weight=V)),
    (UNSUP, dict(pre_scale=V, post_scale=V)), (UNSUP, dict(gate=V, residual=V)),
]


@pytest.mark.parametrize("code,case", REFUSALS, ids=[f"{c}-{'-'.join(k)}" for c, k in REFUSALS])
def test_refusals(code, case):
    assert _call(**case) == code
    assert capi.lib().quip_had_mix_batch_f16(None, 32, 13824, 27, 0, None) == NULL


WIDTHS = [(13824, 27), (18944, 37), (9728, 19), (17408, 17), (25600, 25), (27648, 27), (14336, 28), (28672, 28)]


def test_route():
    for rows in (32, 8192):
        for n, K in WIDTHS:
            assert R.had_mix_batch_route(rows, n, K, n), (rows, n, K)
            assert R.had_mix_batch_route(rows, n, K, n - 40, out_vectors=True, in_features=n)
            assert R.had_mix_batch_route(rows, n, K, n, in_vectors=True, in_features=n - 24)
    for K in (1, 3, 5, 7):
        assert not R.had_mix_batch_route(32, K * 512, K, K * 512)
    assert not R.had_mix_batch_route(31, 13824, 27, 13824)
    assert not R.had_mix_batch_route(32, 27 * 256, 27, 27 * 256) and not R.had_mix_batch_route(32, 8 * 2048, 8, 8 * 2048)
    assert not R.had_mix_batch_route(32, 49 * 512, 49, 49 * 512)
    assert not R.had_mix_batch_route(32, 29 * 1024, 29, 29 * 1024)
    assert not R.had_mix_batch_route(32, 13824, 27, 13824, rms_weight=True)
    assert not R.had_mix_batch_route(32, 13824, 27, 13824, in_vectors=True, out_vectors=True)
    assert not R.had_mix_batch_route(32, 13824, 27, 13820)


def test_switch_is_off_unless_set(monkeypatch):
    monkeypatch.delenv("QUIP_HAD_MIX_BATCH", raising=False)
    monkeypatch.setattr(R, "_HAD_MIX_BATCH", None)
    assert R.had_mix_batch_enabled() is False
