"""The reference's quantizer.py surface: `QuipQuantizer.quantize_model` (calibration data -> per-block
Hessians -> QUIP.quant -> QuantLinear.pack -> save), `convert_model`, `to_dict` / `from_dict`, `save`, and
`load_quantized_model` -- what a user needs to quantise a HF causal LM on one MI355X and to run the
checkpoint through HF transformers with the MI355X QuantLinear.

Same names, arguments, defaults, config-file format and post-load behaviour as the reference
(quantizer.py:59-178 ctor / to_dict / convert_model, :250-715 quantize_model, :718-756 save, :779-848
load_quantized_model).  Not built, and refused by name: dataset loaders by name, fine-tuning
(ft_epochs > 0), merge_suv during quantisation, models dispatched over several devices.

The checkpoint reader is self-contained (torch.load / safetensors, single file or sharded
index) so that loading does not depend on accelerate's dispatch machinery."""
import gc
import json
import logging
import os
from typing import Any, Dict, Iterable, List, Optional, Union

import torch
from torch import nn

from .codebook import codebook_id
from .qlinear import QuantLinear

logger = logging.getLogger(__name__)

QUIP_CONFIG = "quantization_config.json"      # constants.py
BLOCK_PATTERNS = ["transformer.h", "model.decoder.layers", "gpt_neox.layers", "model.layers"]   # constants.py
_CODEBOOKS = ["D4", "E8P12", "HI", "E8P12RVQ3B", "E8P12RVQ4B"]


def _conv1d_type():
    try:
        from transformers.pytorch_utils import Conv1D
        return Conv1D
    except Exception:       # transformers is only needed for the HF model classes
        return ()


def get_layers(module: nn.Module, layers: Optional[List] = None, prefix: Optional[str] = None,
               skip: Optional[List] = None, name: str = "") -> Dict[str, nn.Module]:
    """{qualified name: layer} of every layer of the given types under `prefix`, skipping names that
    contain one of `skip` (utils.py:35-74)."""
    if layers is None:
        layers = [t for t in (_conv1d_type(), nn.Conv2d, nn.Linear) if t != ()]
    skip = skip or []
    if isinstance(module, tuple(layers)):
        if (prefix is None or name.startswith(prefix)) and all(p not in name for p in skip):
            return {name: module}
        return {}
    res = {}
    for n1, child in module.named_children():
        res.update(get_layers(child, layers, prefix, skip, name + "." + n1 if name else n1))
    return res


def get_block_name_with_pattern(model: nn.Module) -> str:
    """name of the module list holding the transformer blocks (utils.py:76-93)"""
    names = [n for n, _ in model.named_modules()]
    for pat in BLOCK_PATTERNS:
        if any(pat in n for n in names):
            return pat
    raise ValueError("Block pattern could not be match. Pass `block_name_to_quantize` argument in `quantize_model`")


def get_preceding_modules(model: nn.Module, module_name: str) -> List[str]:
    """names of the modules that come before `module_name` in registration order (utils.py:96-119): for a HF causal LM
    the embeddings in front of the block list"""
    found, names = False, []

    def walk(mod, prefix):
        nonlocal found
        for child_name, child in mod.named_children():
            full = prefix + "." + child_name if prefix else child_name
            if full == module_name:
                found = True
            if found:
                return
            if module_name.startswith(full + "."):
                walk(child, full)
            else:
                names.append(full)
    walk(model, "")
    return names


def _modules_outside(model: nn.Module, module_name: str) -> List[str]:
    """names of the outermost modules that do not contain `module_name` (everything but the block list)"""
    names = []

    def walk(mod, prefix):
        for child_name, child in mod.named_children():
            full = prefix + "." + child_name if prefix else child_name
            if full == module_name:
                continue
            if module_name.startswith(full + "."):
                walk(child, full)
            else:
                names.append(full)
    walk(model, "")
    return names


def get_seqlen(model: nn.Module) -> int:
    """utils.py:128-138"""
    cfg = model.config.to_dict() if hasattr(model, "config") else {}
    for key in ("max_position_embeddings", "seq_length", "n_positions"):
        if key in cfg:
            return cfg[key]
    return 2048


DATASET_FORMS = ("a list of strings (tokenised with `tokenizer`, packed to model_seqlen)",
                 "a list of token-id sequences or tensors",
                 "a list of dicts with `input_ids` (and optionally `attention_mask`)")


def _ids_row(ids) -> torch.Tensor:
    t = torch.as_tensor(ids).detach().to("cpu", torch.long).reshape(-1)
    if t.numel() == 0:
        raise ValueError("calibration dataset: an empty token sequence")
    return t


def calibration_samples(dataset, tokenizer=None, seqlen: int = 2048) -> List[Dict[str, torch.Tensor]]:
    """The constructor's `dataset` as the reference's sample list (data.py: one {"input_ids", "attention_mask"} of shape
    (1, L <= seqlen) per sample, on the CPU).  Strings are tokenised, joined into one stream and cut into samples of
    seqlen tokens (a rest shorter than seqlen is dropped unless it is all there is); id sequences and dicts are one
    sample each, cut to seqlen."""
    if dataset is None or isinstance(dataset, str):
        raise NotImplementedError(
            f"dataset={dataset!r}: dataset loaders by name (wikitext2, c4, ptb, ... of the reference's data.py) are not "
            "part of this build.  Pass the calibration data itself as " + "; or ".join(DATASET_FORMS) + ".")
    items = list(dataset)
    if not items:
        raise ValueError("calibration dataset is empty; pass " + "; or ".join(DATASET_FORMS))
    seqlen = int(seqlen)
    samples = []
    if all(isinstance(x, str) for x in items):
        if tokenizer is None:
            raise ValueError("a dataset of strings needs a tokenizer")
        stream = []
        for text in items:
            enc = tokenizer(text)
            stream.append(_ids_row(enc["input_ids"] if hasattr(enc, "keys") else enc))
        stream = torch.cat(stream)
        cuts = list(range(0, stream.numel() - seqlen + 1, seqlen)) or [0]
        for lo in cuts:
            ids = stream[lo:lo + seqlen][None]
            samples.append({"input_ids": ids, "attention_mask": torch.ones_like(ids)})
        return samples
    for x in items:
        if isinstance(x, str):
            raise ValueError("calibration dataset mixes strings with other forms")
        if hasattr(x, "keys"):
            if "input_ids" not in x:
                raise ValueError("calibration dataset: a dict without `input_ids`")
            ids = _ids_row(x["input_ids"])[:seqlen][None]
            mask = x.get("attention_mask") if hasattr(x, "get") else None
            mask = torch.ones_like(ids) if mask is None else _ids_row(mask)[:seqlen][None]
            if mask.shape != ids.shape:
                raise ValueError("calibration dataset: attention_mask and input_ids differ in length")
        else:
            ids = _ids_row(x)[:seqlen][None]
            mask = torch.ones_like(ids)
        samples.append({"input_ids": ids, "attention_mask": mask})
    return samples


def calibration_batches(samples, nsamples: int, batch_size: int) -> List[Dict[str, torch.Tensor]]:
    """the first `nsamples` samples in batches of `batch_size` (data.py:27-82); a shorter last batch is kept"""
    if batch_size < 1 or nsamples < 1:
        raise ValueError("nsamples and batch_size must be positive")
    samples = samples[:nsamples]
    batches = []
    for lo in range(0, len(samples), batch_size):
        part = samples[lo:lo + batch_size]
        if len({s["input_ids"].shape[1] for s in part}) != 1:
            raise ValueError(f"calibration samples {lo} .. {lo + len(part) - 1} differ in length: one batch needs "
                             "sequences of one length (pad or cut them, or use batch_size=1)")
        batches.append({k: torch.cat([s[k] for s in part], dim=0) for k in ("input_ids", "attention_mask")})
    return batches


def _to_device(obj, device):
    """tensors inside (nested) tuples / lists / dicts to `device`; everything else as it is"""
    if isinstance(obj, torch.Tensor):
        return obj.to(device)
    if isinstance(obj, tuple):
        return tuple(_to_device(o, device) for o in obj)
    if isinstance(obj, list):
        return [_to_device(o, device) for o in obj]
    if isinstance(obj, dict):
        return {k: _to_device(v, device) for k, v in obj.items()}
    return obj


class _FirstBlockReached(Exception):
    pass


def recurse_getattr(obj, attr: str):
    """utils.py:141-157"""
    for a in attr.split("."):
        obj = obj[int(a)] if isinstance(obj, Iterable) and not isinstance(obj, nn.Module) or \
            isinstance(obj, (nn.ModuleList, nn.Sequential)) else getattr(obj, a)
    return obj


class QuipQuantizer:
    """Configuration holder + model converter (quantizer.py:59-178).  Accepts every constructor
    argument of the reference so that `from_dict(quantization_config)` works on real checkpoints;
    the arguments that only drive the offline quantisation are stored and otherwise unused."""

    def __init__(self, codebook: str, dataset: str = "", nsamples: int = 4096, model_seqlen: int = 2048,
                 quip_tune_iters: int = 10, sigma_reg: float = 0.01, rescale_WH: bool = False, use_rand: bool = True,
                 scale_override: float = -1, opt_resid_scale: float = -1, per_channel: bool = False,
                 block_name_to_quantize: Optional[str] = None,
                 module_name_preceding_first_block: Optional[List[str]] = None, batch_size: int = 4,
                 inference: bool = False, cache_on_gpu: bool = False, modules_to_not_convert: Optional[List] = None,
                 merge_suv: bool = False, ft_epochs: int = 5, *args, **kwargs):
        if codebook not in _CODEBOOKS:
            raise ValueError("Invalid codebook, has to be D4 or E8P12 or HI")          # quantizer.py:124-125
        if ft_epochs > 0 and merge_suv:
            raise ValueError("finetune mode is incompatible with merge_suv")           # quantizer.py:122-123
        if not (0 < sigma_reg < 1):
            raise ValueError("damp_percent must between 0 and 1.")                     # quantizer.py:129-130
        self.dataset, self.nsamples, self.model_seqlen = dataset, nsamples, model_seqlen
        self.quip_tune_iters, self.sigma_reg, self.rescale_WH = quip_tune_iters, sigma_reg, rescale_WH
        self.use_rand, self.scale_override, self.opt_resid_scale = use_rand, scale_override, opt_resid_scale
        self.per_channel, self.block_name_to_quantize = per_channel, block_name_to_quantize
        self.module_name_preceding_first_block = module_name_preceding_first_block
        self.batch_size, self.cache_on_gpu, self.merge_suv = batch_size, cache_on_gpu, merge_suv
        self.modules_to_not_convert = modules_to_not_convert
        self.ft_epochs = ft_epochs
        self.quant_method = "QUiP"
        self.codebook = codebook_id[codebook](inference=inference, opt_resid_scale=opt_resid_scale)

    def to_dict(self) -> Dict[str, Any]:
        """quantization_config.json contents (quantizer.py:132-148)"""
        return {"quant_method": "QUiP", "rescale_WH": self.rescale_WH, "use_rand": self.use_rand,
                "codebook": self.codebook.id, "codesz": self.codebook.codesz,
                "idx_dtype": str(self.codebook.idx_dtype), "merge_suv": self.merge_suv,
                "per_channel": self.per_channel, "opt_resid_scale": self.opt_resid_scale,
                "modules_to_not_convert": self.modules_to_not_convert}

    @classmethod
    def from_dict(cls, config_dict: Dict[str, Any]):
        return cls(**config_dict)                                                      # quantizer.py:150-163

    def _refuse_unbuilt(self, model):
        """everything this build does not do, by name, before the model is touched"""
        if self.dataset is None or isinstance(self.dataset, str):
            calibration_samples(self.dataset)                     # raises NotImplementedError naming the accepted forms
        if self.ft_epochs > 0:
            raise NotImplementedError(
                f"ft_epochs={self.ft_epochs}: block-wise and end-to-end fine-tuning (quantizer.py:500-560, 597-702) are "
                "not part of this build; pass ft_epochs=0")
        if self.merge_suv:
            raise NotImplementedError("merge_suv=True during quantisation (quantizer.py:413-424, 579-595) is not part of "
                                      "this build; pass merge_suv=False (merge_suv checkpoints of the reference still load)")
        if getattr(model, "hf_device_map", None) is not None:
            raise NotImplementedError("the model has an hf_device_map (dispatched over devices / offloaded): quantisation "
                                      "here runs on a single device; load the model without a device_map")

    def capture_first_block_inputs(self, model: nn.Module, batches, device):
        """Run the model on every batch up to its first block and keep what that block is called with: the hidden
        states and every keyword argument (position ids / embeddings, masks, ...), with a forward pre-hook that ends the
        forward there (quantizer.py:325-395).  Kept on the CPU unless cache_on_gpu."""
        if self.block_name_to_quantize is None:
            self.block_name_to_quantize = get_block_name_with_pattern(model)
        if self.module_name_preceding_first_block is None:
            self.module_name_preceding_first_block = get_preceding_modules(model, self.block_name_to_quantize)
        blocks = recurse_getattr(model, self.block_name_to_quantize)
        origin_dtype, origin_device = model.dtype, next(model.parameters()).device
        keep = (lambda t: t) if self.cache_on_gpu else (lambda t: _to_device(t, "cpu"))
        preceding = set(self.module_name_preceding_first_block)
        outside = _modules_outside(model, self.block_name_to_quantize)
        for name in preceding:
            if recurse_getattr(model, name) is None:
                raise ValueError(f"Module {name} was not found in model")
        for name in list(preceding) + [n for n in outside if n not in preceding]:
            mod = recurse_getattr(model, name).to(device)
            if name in preceding:
                mod.float()                # the blocks run in fp32: their input must be fp32
        blocks[0].to(device).float()
        inputs, kwargs_list = [], []

        def store(_, args, kwargs):
            hidden = args[0] if args else kwargs.get("hidden_states")
            if hidden is None:
                raise ValueError("No input value found in the forward pass of the first block")
            inputs.append(keep(hidden))
            kwargs_list.append({k: keep(v) for k, v in kwargs.items() if k != "hidden_states"})
            raise _FirstBlockReached

        handle = blocks[0].register_forward_pre_hook(store, with_kwargs=True)
        try:
            for batch in batches:
                try:
                    model(**{k: v.to(device) for k, v in batch.items()})
                except _FirstBlockReached:
                    pass
        finally:
            handle.remove()
            for name in outside:
                mod = recurse_getattr(model, name)
                if name in preceding:
                    mod.to(origin_dtype)
                mod.to(origin_device)
            blocks[0].to(origin_dtype).to(origin_device)
        if len(inputs) != len(batches):
            raise RuntimeError("the first block was not reached on every calibration batch")
        return inputs, kwargs_list

    @torch.no_grad()
    def quantize_model(self, model: nn.Module, tokenizer: Any = None, save_dir: str = ""):
        """Quantise every linear layer inside the transformer blocks of `model` with the calibration data given to the
        constructor, block by block on one device (quantizer.py:250-715 without fine-tuning):
        capture the first block's inputs; per block, in fp32 on the device: Hessians of every linear from forward hooks
        (QUIP.add_batch), the block's outputs -- taken BEFORE it is quantised -- become the next block's inputs,
        QUIP.quant per linear, the linear replaced by a packed QuantLinear, the block back to the model's dtype and
        device.  Then model.config.quantization_config, `is_quantized`, and `save` / `tokenizer.save_pretrained` when
        save_dir is given.  The returned model runs as load_quantized_model(save_dir) does (same post-load step).
        `dataset`: see calibration_samples; model_seqlen=None takes the model's."""
        from .quip import QUIP
        self._refuse_unbuilt(model)
        if isinstance(tokenizer, str):
            from transformers import AutoTokenizer
            tokenizer = AutoTokenizer.from_pretrained(tokenizer)
        seqlen = self.model_seqlen if self.model_seqlen is not None else get_seqlen(model)
        samples = calibration_samples(self.dataset, tokenizer, seqlen)
        batches = calibration_batches(samples, self.nsamples, self.batch_size)
        if not torch.cuda.is_available():
            raise RuntimeError("No GPU found. A GPU is needed to quantize model.")            # quantizer.py:799-801 likewise
        self.model_seqlen = seqlen
        model.eval()
        has_config = hasattr(model, "config")
        if has_config:
            use_cache = getattr(model.config, "use_cache", None)
            model.config.use_cache = False
        origin_dtype, origin_device = model.dtype, next(model.parameters()).device
        device = origin_device if origin_device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
        layer_inputs, layer_kwargs = self.capture_first_block_inputs(model, batches, device)
        blocks = recurse_getattr(model, self.block_name_to_quantize)
        torch.cuda.empty_cache()
        for i, block in enumerate(blocks):
            logger.info("quantizing block %s %d/%d", self.block_name_to_quantize, i + 1, len(blocks))
            block = block.to(device).float()
            layers = get_layers(block, skip=self.modules_to_not_convert)
            quant_method = {name: QUIP(layer, self.codebook) for name, layer in layers.items()}
            handles = [layer.register_forward_hook(
                lambda _, inp, out, name=name: quant_method[name].add_batch(inp[0].data, out.data))
                for name, layer in layers.items()]
            layer_outputs = []
            try:
                for hidden, kwargs in zip(layer_inputs, layer_kwargs):
                    out = block(_to_device(hidden, device), **_to_device(kwargs, device))
                    out = out[0] if isinstance(out, (tuple, list)) else out
                    layer_outputs.append(out if self.cache_on_gpu else out.cpu())
            finally:
                for h in handles:
                    h.remove()
            attrs = {}
            for name in layers:
                attrs[name] = quant_method[name].quant(
                    rescale_WH=self.rescale_WH, sigma_reg=self.sigma_reg, quip_tune_iters=self.quip_tune_iters,
                    scale_override=self.scale_override, use_rand=self.use_rand, per_channel=self.per_channel)
                quant_method[name].free()
            self._replace_by_quant_layers(block, set(layers))
            for name, layer in layers.items():
                quant_layer = recurse_getattr(block, name)
                quant_layer.pack(layer, attrs[name])
                quant_layer.train(block.training)        # a new module starts in training mode; the model is in eval()
                layer.to("cpu")
                quant_layer.to(device)
            blocks[i] = block.to(origin_dtype).to(origin_device)
            for name in layers:
                quant_layer = recurse_getattr(blocks[i], name)
                quant_layer.weight_dtype = origin_dtype
                if not self.per_channel:      # the scalar scale stays fp32, as in a loaded checkpoint
                    quant_layer.Wscale = attrs[name]["w_scale"].to(torch.float32).reshape(()).to(origin_device)
            del layers, quant_method, attrs
            layer_inputs, layer_outputs = layer_outputs, []
            gc.collect()
            torch.cuda.empty_cache()
        del layer_inputs, layer_kwargs
        model.is_quantized = True
        if has_config:
            model.config.use_cache = use_cache
            model.config.quantization_config = self.to_dict()
        if save_dir:
            self.save(model, save_dir)
            if tokenizer is not None:
                tokenizer.save_pretrained(save_dir)
        # what load_quantized_model does after filling the layers (the saved tensors are the un-finalised ones)
        finalize_quant_layers(model, merge_suv=False)
        torch.cuda.empty_cache()
        return model

    def convert_model(self, model: nn.Module) -> nn.Module:
        """replace every linear layer inside the transformer blocks by an (empty) QuantLinear
        (quantizer.py:165-178, 195-248)"""
        if self.block_name_to_quantize is None:
            self.block_name_to_quantize = get_block_name_with_pattern(model)
        names = get_layers(model, prefix=self.block_name_to_quantize, skip=self.modules_to_not_convert)
        self._replace_by_quant_layers(model, set(names))
        return model

    def get_no_split_module_classes(self, model) -> List[str]:
        return [recurse_getattr(model, self.block_name_to_quantize)[0].__class__.__name__]   # quantizer.py:180-193

    def _replace_by_quant_layers(self, module: nn.Module, names, name: str = ""):
        if isinstance(module, QuantLinear):
            return
        conv1d = _conv1d_type()
        for attr, layer in list(module.named_children()):
            full = name + "." + attr if name else attr
            if full in names:
                if isinstance(layer, nn.Linear):
                    fin, fout = layer.in_features, layer.out_features
                elif isinstance(layer, nn.Conv2d):
                    fin, fout = layer.in_channels, layer.out_channels
                elif conv1d != () and isinstance(layer, conv1d):
                    fin, fout = layer.weight.shape[0], layer.weight.shape[1]
                else:
                    continue
                device = layer.weight.device
                cb = codebook_id[self.codebook.id](inference=True, opt_resid_scale=self.opt_resid_scale)
                new = QuantLinear(fin, fout, cb, bias=(layer.bias is not None), use_rand=self.use_rand,
                                  per_channel=self.per_channel, weight_dtype=layer.weight.dtype)
                new.device = device
                if device != torch.device("meta"):
                    new = new.to(device)
                setattr(module, attr, new)
            else:
                self._replace_by_quant_layers(layer, names, full)

    def save(self, model: nn.Module, save_dir: str, max_shard_size: str = "10GB", safe_serialization: bool = False):
        """state dict + model config + quantization_config.json (quantizer.py:718-756).  Same on-disk layout as
        the reference's `Accelerator.save_model`: `pytorch_model.bin` / `model.safetensors`, or, when the state dict
        exceeds `max_shard_size`, `pytorch_model-0000i-of-0000N.bin` (`model-...safetensors`) plus the
        `*.index.json` weight map.  Tensors that share storage (tied embeddings) are written once for
        safetensors; `load_quantized_model` re-ties them."""
        os.makedirs(save_dir, exist_ok=True)
        sd, seen = {}, {}
        for k, v in model.state_dict().items():
            v = v.detach()
            if safe_serialization and v.numel() > 0:
                key = (v.device, v.data_ptr(), tuple(v.shape), tuple(v.stride()), v.dtype)
                if key in seen:
                    continue                 # tied weight: keep the first name only
                seen[key] = k
            sd[k] = v.cpu().contiguous()
        limit = _parse_size(max_shard_size)
        shards, cur, cur_bytes = [], {}, 0
        for k, v in sd.items():
            nbytes = v.numel() * v.element_size()
            if cur and cur_bytes + nbytes > limit:
                shards.append(cur)
                cur, cur_bytes = {}, 0
            cur[k] = v
            cur_bytes += nbytes
        shards.append(cur)
        base, ext = ("model", ".safetensors") if safe_serialization else ("pytorch_model", ".bin")

        def write(tensors, path):
            if safe_serialization:
                from safetensors.torch import save_file
                save_file(tensors, path, metadata={"format": "pt"})
            else:
                torch.save(tensors, path)
        if len(shards) == 1:
            write(shards[0], os.path.join(save_dir, base + ext))
        else:
            weight_map = {}
            for i, sh in enumerate(shards):
                name = f"{base}-{i + 1:05d}-of-{len(shards):05d}{ext}"
                write(sh, os.path.join(save_dir, name))
                weight_map.update({k: name for k in sh})
            total = sum(v.numel() * v.element_size() for v in sd.values())
            with open(os.path.join(save_dir, base + ext + ".index.json"), "w", encoding="utf-8") as f:
                json.dump({"metadata": {"total_size": total}, "weight_map": weight_map}, f, indent=2, sort_keys=True)
        if hasattr(model, "config"):
            model.config.save_pretrained(save_dir)
        with open(os.path.join(save_dir, QUIP_CONFIG), "w", encoding="utf-8") as f:
            json.dump(self.to_dict(), f, indent=2)


def _parse_size(size) -> int:
    """'10GB' / '300KB' / '5MiB' / int -> bytes (the size strings accelerate / huggingface_hub accept)"""
    if isinstance(size, int):
        return size
    s = str(size).strip().upper()
    units = [("GIB", 2 ** 30), ("MIB", 2 ** 20), ("KIB", 2 ** 10), ("GB", 10 ** 9), ("MB", 10 ** 6), ("KB", 10 ** 3),
             ("B", 1)]
    for u, m in units:
        if s.endswith(u):
            return int(float(s[:-len(u)]) * m)
    return int(s)


def _checkpoint_files(folder: str) -> List[str]:
    """weight files of a HF-style checkpoint directory (single file or sharded index)"""
    for index in ("model.safetensors.index.json", "pytorch_model.bin.index.json"):
        p = os.path.join(folder, index)
        if os.path.exists(p):
            with open(p) as f:
                return sorted({os.path.join(folder, v) for v in json.load(f)["weight_map"].values()})
    for single in ("model.safetensors", "pytorch_model.bin"):
        p = os.path.join(folder, single)
        if os.path.exists(p):
            return [p]
    raise FileNotFoundError(f"no model weights (model.safetensors / pytorch_model.bin [+ index]) in {folder}")


def load_state_dict_from_folder(folder: str) -> Dict[str, torch.Tensor]:
    sd = {}
    for p in _checkpoint_files(folder):
        if p.endswith(".safetensors"):
            from safetensors.torch import load_file
            sd.update(load_file(p))
        else:
            sd.update(torch.load(p, map_location="cpu", weights_only=True))
    return sd


def finalize_quant_layers(model: nn.Module, merge_suv: bool = False):
    """the reference's post-load step (quantizer.py:833-844): scalar Wscale folded into the input
    transform, per-channel scales normalised, all-positive SU / SV dropped for merge_suv models"""
    for layer in get_layers(model, [QuantLinear]).values():
        layer.wscale_float = layer.Wscale.mean().float().item()
        if layer.per_channel:
            layer.Wscale = layer.Wscale / layer.Wscale.mean()
        if merge_suv:
            if torch.all(layer.SU > 0):
                layer.SU = None
            if torch.all(layer.SV > 0):
                layer.SV = None


def load_quantized_model(save_folder: str, revision: Optional[str] = None,
                         torch_dtype: Optional[Union[str, torch.dtype]] = torch.float16,
                         trust_remote_code: bool = True, use_safetensors: bool = False,
                         device_map: Optional[Union[str, Dict]] = None, _require_gpu: bool = True,
                         fast_decode: Optional[bool] = None):
    """Load a QuIP-for-all checkpoint directory into a HF causal LM whose linear layers are
    QuantLinear (quantizer.py:779-848).  Like the reference: needs a GPU (raises otherwise),
    default device_map leaves the weights on the CPU ({"": "cpu"}), the model comes back in eval
    mode with `is_quantized = True`.  device_map may also be a device string or {"": device}.
    fast_decode (not in the reference; default on, QUIP_FAST_DECODE=0 or fast_decode=False switches it off): single-token
    forward calls on an initialised transformers StaticCache -- the reference's decode loop, example_generate.py:28-33, and
    `generate(cache_implementation="static")` -- run the fused decoder on the same modules and cache tensors (hf_fast.py);
    every other call is the stock forward.  QUIP_FAST_DECODE_BATCH=1 also routes decode steps of left-padded `generate`
    batches through the batched decoder (off by default; hf_fast.py, BATCHES, for what it serves and what its buffers cost)."""
    if _require_gpu and not torch.cuda.is_available():
        raise RuntimeError("No GPU found. A GPU is needed to run quantized model.")          # quantizer.py:799-801
    if not os.path.isdir(save_folder):
        raise FileNotFoundError(f"{save_folder} is not a directory (hub download is not available: no network)")
    from transformers import AutoConfig, AutoModelForCausalLM
    config = AutoConfig.from_pretrained(save_folder, trust_remote_code=trust_remote_code, revision=revision)
    if isinstance(torch_dtype, str):
        torch_dtype = getattr(torch, torch_dtype)
    # parameters on the meta device, buffers real (rotary inv_freq, causal masks, ... are computed by the model's
    # constructor and are not in the checkpoint): what the reference's init_empty_weights(include_buffers=False)
    # does (quantizer.py:805-809)
    with _params_on_meta():
        model = AutoModelForCausalLM.from_config(config, trust_remote_code=trust_remote_code, dtype=torch_dtype)
    qcfg = getattr(config, "quantization_config", None)
    if qcfg is None:
        with open(os.path.join(save_folder, QUIP_CONFIG)) as f:
            qcfg = json.load(f)
    qcfg = dict(qcfg)
    qcfg.pop("quant_method", None)
    qcfg.pop("codesz", None)
    qcfg.pop("idx_dtype", None)
    qcfg["inference"] = True
    qcfg["ft_epochs"] = 0
    quantizer = QuipQuantizer.from_dict(qcfg)
    model = quantizer.convert_model(model)
    # materialise the meta parameters on the CPU (the QuantLinear buffers and codebook tables are real
    # already and must be kept), then fill from the checkpoint
    was_meta = _materialize_meta(model)
    sd = load_state_dict_from_folder(save_folder)
    own = model.state_dict()
    missing = [k for k in own if k not in sd]

    def soft(k):
        # the fake 0-dim `weight` of a QuantLinear; SU / SV of layers packed with merge_su / merge_sv (the reference
        # drops those parameters, qlinear.py:117-131, loads non-strictly and leaves them at their init of ones,
        # which the post-load step then removes); a tied lm_head
        # Only a merge_suv checkpoint may lack SU / SV: without it a missing SU / SV means a truncated or renamed
        # checkpoint, and filling it with ones would load a model that silently computes something else.
        stem, _, leaf = k.rpartition(".")
        if stem + ".Qidxs" in own and (leaf == "weight" or (leaf in ("SU", "SV") and bool(quantizer.merge_suv))):
            return True
        return k == "lm_head.weight" and bool(getattr(config, "tie_word_embeddings", False))
    hard_missing = [k for k in missing if not soft(k) and (k in was_meta or k.rpartition(".")[0] + ".Qidxs" in own)]
    if hard_missing:
        raise KeyError(f"checkpoint lacks {len(hard_missing)} tensors, e.g. {hard_missing[:5]}")
    cast = {}
    for k, v in sd.items():
        if k in own:
            cast[k] = v.to(own[k].dtype) if v.is_floating_point() and own[k].is_floating_point() else v
    model.load_state_dict(cast, strict=False)
    for k in missing:                      # merge_suv layers: SU / SV stay at ones
        stem, _, leaf = k.rpartition(".")
        if leaf in ("SU", "SV") and stem + ".Qidxs" in own:
            getattr(recurse_getattr(model, stem), leaf).data.fill_(1.0)
    if hasattr(model, "tie_weights") and ("lm_head.weight" in missing or getattr(config, "tie_word_embeddings", False)):
        model.tie_weights()                # materialising the meta parameters untied them
    left = [n for n, t in list(model.named_parameters()) + list(model.named_buffers()) if t.is_meta]
    if left:
        raise RuntimeError(f"tensors left on the meta device after loading: {left[:5]}")
    finalize_quant_layers(model, merge_suv=quantizer.merge_suv)
    if device_map is not None:
        dev = device_map if isinstance(device_map, (str, torch.device)) else device_map.get("", "cpu")
        if dev == "auto":
            dev = "cuda:0"
        model = model.to(dev)
    model.is_quantized = True
    model.eval()
    if fast_decode is None:
        fast_decode = os.environ.get("QUIP_FAST_DECODE", "1") != "0"
    if fast_decode:
        from .hf_fast import enable_fast_decode
        enable_fast_decode(model, batch=os.environ.get("QUIP_FAST_DECODE_BATCH", "0") != "0")
    return model


class _params_on_meta:
    """Context in which nn.Module parameters are created on the meta device while buffers stay real -- the
    behaviour of accelerate.init_empty_weights(include_buffers=False) that the reference relies on
    (quantizer.py:805), without depending on accelerate."""

    def __enter__(self):
        self._orig = nn.Module.register_parameter

        def register_parameter(module, name, param):
            self._orig(module, name, param)
            if param is not None and not param.is_meta:
                cls = type(module._parameters[name])
                kw = dict(module._parameters[name].__dict__)
                kw["requires_grad"] = param.requires_grad
                module._parameters[name] = cls(module._parameters[name].to(torch.device("meta")), **kw)
        nn.Module.register_parameter = register_parameter
        return self

    def __exit__(self, *exc):
        nn.Module.register_parameter = self._orig
        return False


def _materialize_meta(model: nn.Module, device="cpu"):
    """zero tensors for everything still on the meta device; returns the qualified names it replaced (parameters
    only after _params_on_meta; buffers too for models built under torch.device('meta'))"""
    replaced = set()
    for mname, m in model.named_modules():
        pre = mname + "." if mname else ""
        for name, p in list(m._parameters.items()):
            if p is not None and p.is_meta:
                m._parameters[name] = nn.Parameter(torch.zeros(p.shape, dtype=p.dtype, device=device),
                                                   requires_grad=p.requires_grad)
                replaced.add(pre + name)
        for name, b in list(m._buffers.items()):
            if b is not None and b.is_meta:
                m._buffers[name] = torch.zeros(b.shape, dtype=b.dtype, device=device)
                replaced.add(pre + name)
    return replaced
