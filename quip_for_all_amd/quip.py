"""Layer-level quantiser with the reference's class name and attr contract (quip.py:17-200): accumulate
the proxy Hessian of one nn.Linear from calibration inputs, incoherence-process (random signs + randomised
Hadamard on both sides), LDLQ-round against a codebook, and hand back what QuantLinear.pack() consumes.
Host logic in torch; LDLQ for E8P12 rounds a panel of 128 columns per launch (quant.LDLQ_panels, csrc/quantize.hip), the
other codebooks go through cb.quantize() per column group.  QuipQuantizer.quantize_model drives this class over a model."""
import itertools
import math
import os

import torch
import torch.nn as nn

from .quant import LDLQ, get_hadK, incoherence_in, incoherence_out, parse_ldlq_fused

_HESSIAN_FUSED = None
HESSIAN_FUSED_DTYPES = (torch.float16, torch.bfloat16, torch.float32)


def hessian_fused_enabled():
    """QUIP_HESSIAN_FUSED, off unless set; read once per process.  On: QUIP.add_batch accumulates CUDA inputs of
    HESSIAN_FUSED_DTYPES with one torch.ops.quip_lib.hessian_accumulate launch (csrc/hessian.hip), and quantize_model
    accumulates a tensor that several modules of a block receive once (SharedHessianInputs).  The launch scales the sum
    X^T X by 2 / nsamples where the torch expression scales x by sqrt(2 / nsamples) first: the two routes agree to
    rounding, not bit for bit."""
    global _HESSIAN_FUSED
    if _HESSIAN_FUSED is None:
        _HESSIAN_FUSED = parse_ldlq_fused(os.environ.get("QUIP_HESSIAN_FUSED"), default=False)
    return _HESSIAN_FUSED


_history = itertools.count(1)


def tensor_identity(t):
    """what two tensors share when they are the same values at the same place: storage pointer, offset, shape, strides, dtype,
    device and version counter.  Only meaningful while both tensors are alive: a freed tensor's address is handed out again."""
    return (t.untyped_storage().data_ptr(), t.storage_offset(), tuple(t.shape), t.stride(), t.dtype, t.device, t._version)


class SharedHessianInputs:
    """The forward hooks of one block: modules that receive the same tensor (q / k / v_proj, gate / up_proj) accumulate it
    once, the later ones copy H and mu from the module that did the work -- n^2 elements of traffic against n^2 rows
    operations.  The last input stays referenced until the next one arrives, so its identity cannot be another tensor's; a
    module copies only from a donor of equal columns whose H, mu and nsamples were its own before the donor's update (the
    history token of QUIP).  Every QUIP keeps its own H."""

    def __init__(self):
        self.copies = 0         # accumulations answered by a copy
        self.forget()

    def forget(self):
        """drop the reference to the last input"""
        self._inp = self._key = self._donor = self._before = None

    def add_batch(self, quip, inp, out=None):
        """quip.add_batch(inp.data, out), or its result copied from the module that has just accumulated the same tensor"""
        key = tensor_identity(inp)
        donor = self._donor
        if (self._inp is not None and key == self._key and donor is not quip and donor.columns == quip.columns
                and quip.history == self._before):
            quip.H.copy_(donor.H)
            quip.mu.copy_(donor.mu)
            quip.nsamples, quip.history = donor.nsamples, donor.history
            self.copies += 1
            return
        before = quip.history
        quip.add_batch(inp.data, out)
        self._inp, self._key, self._donor, self._before = inp, key, quip, before


class QUIP:
    def __init__(self, layer, cb):
        assert isinstance(layer, nn.Linear), "this build quantises nn.Linear layers"
        self.layer = layer
        self.dev = layer.weight.device
        self.rows, self.columns = layer.weight.shape
        self.H = torch.zeros((self.columns, self.columns), dtype=torch.float64, device=self.dev)
        self.mu = torch.zeros((self.columns,), dtype=torch.float64, device=self.dev)
        self.nsamples = 0
        self.history = 0        # equal tokens: equal H, mu and nsamples (0: nothing accumulated; SharedHessianInputs)
        self.cb = cb.to(self.dev)

    def add_batch(self, inp, out=None):
        """running mean of 2 x x^T over the calibration rows (quip.py:40-69)"""
        self.history = next(_history)
        batch = 1 if inp.dim() == 2 else inp.shape[0]
        if hessian_fused_enabled() and inp.is_cuda and inp.dtype in HESSIAN_FUSED_DTYPES:
            x = inp.reshape(-1, inp.shape[-1])
            if x.is_contiguous() and x.shape[0] >= 1 and self.columns >= 8 and self.columns % 8 == 0:
                ns = self.nsamples + batch
                torch.ops.quip_lib.hessian_accumulate(self.H, self.mu, x, self.nsamples / ns, 2 / ns, 1 / ns)
                self.nsamples = ns
                return
        x = inp.reshape(-1, inp.shape[-1]).to(torch.float64).t()            # (columns, rows)
        keep = self.nsamples / (self.nsamples + batch)
        self.H *= keep
        self.mu *= keep
        self.nsamples += batch
        self.mu += x.sum(dim=1) / self.nsamples
        x = math.sqrt(2 / self.nsamples) * x
        self.H += x @ x.t()

    def quant(self, rescale_WH=False, use_fp64=False, sigma_reg=0.01, scale_override=0, use_buffered=True,
              use_rand=True, per_channel=False, quip_tune_iters=0):
        """returns the attr dict of quip.py:176-187 and leaves the de-rotated hatW in layer.weight (the free
        end-to-end golden: nn.Linear(hatW)(x) == QuantLinear(x), SURVEY 4 identity 3)"""
        H = self.H.clone() if use_fp64 else self.H.to(torch.float32)
        if self.nsamples == 0:       # no calibration data: identity proxy (plain nearest rounding + LDL = I)
            H = torch.eye(self.columns, dtype=H.dtype, device=self.dev)
        w = self.layer.weight.data.clone().to(H.dtype)
        dead = torch.diag(H) == 0
        H[dead, dead] = 1
        w[:, dead] = 0
        H = H / torch.diag(H).mean()
        scaleWH = None
        if rescale_WH:
            H = H / H.abs().max()
            dH = torch.diag(H).clamp(min=1e-8)
            dW = torch.diag(w.T @ w).clamp(min=1e-8)
            scaleWH = (dH / dW).sqrt().sqrt().to(torch.float32).clamp(min=1e-8)
            w = w * scaleWH[None, :]
            H = H / scaleWH[None, :] / scaleWH[:, None]
        merge_su, merge_sv = hasattr(self.layer, "SU"), hasattr(self.layer, "SV")
        rsign = lambda k: (torch.randn(k, device=self.dev).sign() + 1e-5).sign().to(H.dtype)   # noqa: E731
        SU = self.layer.SU.to(H.dtype) if merge_su else rsign(self.columns)
        SV = self.layer.SV.to(H.dtype) if merge_sv else rsign(self.rows)
        lhad, lK, lN = get_hadK(self.columns, use_rand=use_rand)
        rhad, rK, rN = get_hadK(self.rows, use_rand=use_rand)
        # incoherence processing: H <- U_L (SU H SU) U_L^T,  W <- U_R (SV W SU) U_L^T   (quip.py:124-128)
        H, w = incoherence_in(H, w, SU, SV, lhad, lK, lN, rhad, rK, rN)
        diag = torch.arange(H.shape[0], device=self.dev)
        for attempt in range(10):
            H[diag, diag] += sigma_reg
            try:
                L = torch.linalg.cholesky(H)
                if not torch.isnan(L).any():
                    break
            except RuntimeError:
                pass
        else:
            raise ValueError("Hessian is not invertible")
        w_scale = w.square().mean(dim=1, keepdim=True).sqrt() if per_channel else w.square().mean().sqrt()
        w_scale = w_scale / (scale_override if scale_override > 0 else self.cb.opt_scale)
        hat_w, Qidxs = LDLQ(w / w_scale, H, L, self.cb, quip_tune_iters, buf_cols=128 if use_buffered else self.cb.codesz)
        hat_w = hat_w * w_scale
        # back to the original basis (quip.py:162-167)
        deq = incoherence_out(hat_w, SU, SV, lhad, lK, lN, rhad, rK, rN, self.columns, self.rows)
        if rescale_WH:
            deq = deq / scaleWH[None, :]
        self.layer.weight.data = deq.reshape(self.layer.weight.shape).to(self.layer.weight.dtype)
        return {
            "left_hadK": lhad.cpu() if use_rand and lhad is not None else None,
            "right_hadK": rhad.cpu() if use_rand and rhad is not None else None,
            "Qidxs": self.cb.maybe_pack_idxs(Qidxs).cpu(),
            "w_scale": w_scale.cpu(),
            "SU": SU.cpu(), "SV": SV.cpu(),
            "merge_su": merge_su, "merge_sv": merge_sv,
            "scaleWH": scaleWH.cpu() if rescale_WH else None,
        }

    def free(self):
        self.H = self.mu = None
        torch.cuda.empty_cache()
