"""quip_lib::hessian_accumulate (csrc/hessian.hip) and QUIP.add_batch on it behind QUIP_HESSIAN_FUSED: equality on operands whose
every product and sum is exact in fp64, the summation bound against float64 on the CPU otherwise."""
import pytest
import torch
from torch import nn

from quip_for_all_amd import quip
from quip_for_all_amd.register_lib import hessian_row_block

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KB = hessian_row_block()
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
U = 2.0 ** -53


def _reference(H, mu, X, keep, s_h, s_mu):
    """float64 on the CPU, and the magnitudes the summation bound scales with"""
    x = X.cpu().double()
    ref = keep * H + s_h * (x.t() @ x), keep * mu + s_mu * x.sum(0)
    mag = s_h * (x.abs().t() @ x.abs()) + keep * H.abs(), s_mu * x.abs().sum(0) + keep * mu.abs()
    return ref, mag


def _exact_run(n, rows, dtype):
    g = torch.Generator().manual_seed(1000 * n + rows)
    ints = [torch.randint(-64, 65, (rows, n), generator=g) for _ in range(2)]
    H = torch.zeros(n, n, dtype=torch.float64, device=DEV)
    mu = torch.zeros(n, dtype=torch.float64, device=DEV)
    for xi, (keep, s_h, s_mu) in zip(ints, ((0.0, 1.0, 0.5), (0.5, 0.5, 0.25))):
        torch.ops.quip_lib.hessian_accumulate(H, mu, (xi / 8.0).to(dtype).to(DEV), keep, s_h, s_mu)
    return ints, H.cpu(), mu.cpu()


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("rows", [1, 3, KB - 1, KB + 1, 300])
@pytest.mark.parametrize("n", [8, 120, 128, 136, 688])
def test_exact_operands_give_equal_results(n, rows, dtype):
    (a, b), H, mu = _exact_run(n, rows, DTYPES[dtype])
    want_H = 0.5 * ((a.t() @ a).double() / 64.0) + 0.5 * ((b.t() @ b).double() / 64.0)        # int64 products, exact
    want_mu = 0.5 * (0.5 * a.sum(0).double() / 8.0) + 0.25 * b.sum(0).double() / 8.0
    assert torch.equal(H, want_H) and torch.equal(mu, want_mu)
    assert torch.equal(H, H.t())
    _, H2, mu2 = _exact_run(n, rows, DTYPES[dtype])
    assert torch.equal(H, H2) and torch.equal(mu, mu2)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("rows,n", [(300, 688), (257, 136)])
def test_random_operands_inside_the_summation_bound(rows, n, dtype):
    g = torch.Generator().manual_seed(rows + n)
    X = torch.randn(rows, n, generator=g).to(DTYPES[dtype])
    H0 = torch.randn(n, n, generator=g, dtype=torch.float64)
    H0, mu0 = H0 + H0.t(), torch.randn(n, generator=g, dtype=torch.float64)
    keep, s_h, s_mu = 0.75, 2 / 7, 1 / 7
    H, mu = H0.clone().to(DEV), mu0.clone().to(DEV)
    torch.ops.quip_lib.hessian_accumulate(H, mu, X.to(DEV), keep, s_h, s_mu)
    (want_H, want_mu), (mag_H, mag_mu) = _reference(H0, mu0, X, keep, s_h, s_mu)
    err_H, err_mu = (H.cpu() - want_H).abs(), (mu.cpu() - want_mu).abs()
    print("max err / bound: H %.3g mu %.3g" % ((err_H / (2 * (rows + 8) * U * mag_H)).max(),
                                               (err_mu / (2 * (rows + 8) * U * mag_mu)).max()))
    assert (err_H <= 2 * (rows + 8) * U * mag_H).all() and (err_mu <= 2 * (rows + 8) * U * mag_mu).all()
    assert torch.equal(H, H.t())


def test_add_batch_takes_the_launch_only_behind_the_switch(monkeypatch):
    calls, op = [], torch.ops.quip_lib.hessian_accumulate
    monkeypatch.setattr(torch.ops.quip_lib, "hessian_accumulate", lambda *a: (calls.append(1), op(*a))[1])
    g = torch.Generator().manual_seed(5)
    batches = [torch.randn(4, 64, 136, generator=g).to(DEV) for _ in range(3)]
    runs = {}
    for fused in (False, True):
        monkeypatch.setattr(quip, "_HESSIAN_FUSED", fused)
        q = quip.QUIP(nn.Linear(136, 8).to(DEV), nn.Identity())
        for x in batches:
            q.add_batch(x)
        runs[fused] = q
        assert len(calls) == (3 if fused else 0)
    assert runs[True].nsamples == runs[False].nsamples == 12
    x = torch.cat(batches).reshape(-1, 136).cpu().double().abs()
    rows = x.shape[0]
    assert ((runs[True].H - runs[False].H).abs().cpu() <= 2 * (rows + 8) * U * (2 / 12) * (x.t() @ x)).all()
    assert ((runs[True].mu - runs[False].mu).abs().cpu() <= 2 * (rows + 8) * U * (1 / 12) * x.sum(0)).all()
