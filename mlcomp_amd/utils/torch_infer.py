"""Inference helpers (`mlcomp/utils/torch.py:11-71`): run a traced model file over a
dataset (optionally batch-by-batch), apply an activation, undo TTA.

On the GPU the model runs under bf16 autocast with channels-last inputs (MIOpen/
hipBLASLt pick their NHWC kernels); logits come back as fp32 numpy.
"""
from __future__ import annotations

from typing import Iterator, Optional

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset


def apply_activation(x: torch.Tensor, activation: Optional[str]):
    if not activation:
        return x
    if activation == 'sigmoid':
        return torch.sigmoid(x)
    if activation == 'softmax':
        return torch.softmax(x, 1)
    raise ValueError(f'unknown activation = {activation}')


def _device():
    return torch.device('cuda') if torch.cuda.is_available() else torch.device('cpu')


def load_model(file: str, device=None):
    dev = device or _device()
    try:
        m = torch.jit.load(file, map_location=dev)
    except RuntimeError:
        raise RuntimeError(f'{file} is not a TorchScript model (export it with trace / model_add)')
    return m.eval()


def _collate(batch):
    from mlcomp_amd.train.data import collate_dict
    return collate_dict(batch)


def _batches(model, loader, activation, dev) -> Iterator[dict]:
    from mlcomp_amd.contrib.transform.tta import TtaWrap
    use_amp = dev.type == 'cuda'
    with torch.no_grad():
        for batch in loader:
            x = batch['features'].to(dev, non_blocking=True).float()
            if x.dim() == 4 and use_amp:
                x = x.contiguous(memory_format=torch.channels_last)
            with torch.autocast(dev.type, dtype=torch.bfloat16, enabled=use_amp):
                logits = model(x)
            p = apply_activation(logits.float(), activation)
            if isinstance(loader.dataset, TtaWrap):
                p = loader.dataset.inverse(p)
            p = p.cpu().numpy()
            yield {'prob': p, 'count': p.shape[0], **batch}


def _native_model(model, checkpoint, model_spec, dev):
    """The nn.Module the native engine lowers, or NativeUnsupported with the reason."""
    from mlcomp_amd.train.native_infer import NO_DEVICE, unsupported_reason
    from mlcomp_amd.train.native_spec import NativeUnsupported
    if dev.type != 'cuda':
        raise NativeUnsupported(NO_DEVICE)
    if (model is None or isinstance(model, torch.jit.ScriptModule)) and checkpoint and model_spec:
        from mlcomp_amd.models import build_model
        spec = dict(model_spec)
        model = build_model(spec.pop('name'), **spec)
        ck = torch.load(checkpoint, map_location='cpu', weights_only=True)
        model.load_state_dict(ck.get('model_state_dict', ck))
    reason = unsupported_reason(model)
    if reason is not None:
        raise NativeUnsupported(reason)
    return model


def _native_engine(engines: dict, model, batch_size, x, dev):
    """The NativeInference engine for batches of ``x``'s image size out of ``engines`` (the
    caller's cache; built and stored there when missing), or NativeUnsupported."""
    from mlcomp_amd.train.native_infer import NativeInference
    from mlcomp_amd.train.native_spec import NativeUnsupported
    if x.dim() != 4 or x.shape[1] not in (1, 3):
        raise NativeUnsupported(f'features of shape {tuple(x.shape)}: the native engine takes NCHW images')
    key = (int(batch_size), int(x.shape[2]), int(x.shape[3]))
    if key not in engines:
        engines[key] = NativeInference(model, key[0], key[1:], device=dev)
    return engines[key]


def _native_batches(model, loader, activation, dev, batch_size, engines) -> Iterator[dict]:
    """As :func:`_batches`, with the logits from :class:`NativeInference` engines."""
    from mlcomp_amd.contrib.transform.tta import TtaWrap
    from mlcomp_amd.train.native_spec import NativeUnsupported
    for batch in loader:
        x = batch['features']
        try:
            eng = _native_engine(engines, model, batch_size, x, dev)
        except NativeUnsupported as e:     # a later batch of another kind than the first
            raise RuntimeError(f'engine: native cannot run this batch: {e}')
        logits = eng.predict(x.float())
        p = apply_activation(logits.float(), activation)
        if isinstance(loader.dataset, TtaWrap):
            p = loader.dataset.inverse(p)
        p = p.cpu().numpy()
        yield {'prob': p, 'count': p.shape[0], **batch}


def infer(x: Dataset, file: str, batch_size: int = 1, batch_mode: bool = False, activation=None,
          num_workers: int = 0, model=None, engine: str = 'torch', checkpoint: str = None, model_spec: dict = None,
          engines: dict = None):
    """``engine='torch'`` (default): the TorchScript file / ``model`` under bf16 autocast.
    ``engine='native'``: the hand-written kernels (:class:`NativeInference`); needs ``model`` as
    an nn.Module, or ``checkpoint`` plus ``model_spec`` (``build_model`` arguments), and raises
    with the reason when it cannot run.  ``engine='auto'``: native when possible, else the
    torch path with the reason logged.  The engine folds the module's weights as they are at
    this call; ``engines`` (a dict the caller owns) keeps the built engines for later calls
    with the same, unchanged module - without it every call builds its own."""
    if engine not in ('torch', 'native', 'auto'):
        raise ValueError(f'engine: torch / native / auto, not {engine!r}')
    dev = _device()
    loader = DataLoader(x, batch_size=batch_size, shuffle=False, num_workers=num_workers,
                        pin_memory=dev.type == 'cuda', collate_fn=_collate)
    it = None
    if engine != 'torch' and len(x):
        from mlcomp_amd.train.native_spec import NativeUnsupported
        try:
            # everything that can decline is decided here, before the first batch: the device,
            # the model's lowering, the kind of the data and the engine's construction
            native = _native_model(model, checkpoint, model_spec, dev)
            engines = engines if engines is not None else {}
            first = torch.as_tensor(x[0]['features'])
            _native_engine(engines, native, batch_size, first[None], dev)
            it = _native_batches(native, loader, activation, dev, batch_size, engines)
        except NativeUnsupported as e:
            if engine == 'native':
                raise RuntimeError(f'engine: native cannot run this model: {e}')
            import logging
            logging.getLogger(__name__).warning('engine: auto runs the torch path: %s', e)
    if it is None:
        model = model if model is not None else load_model(file, dev)
        if engine != 'torch' and not isinstance(model, torch.jit.ScriptModule):
            model = model.to(dev).eval()      # the module the native engine declined
        it = _batches(model, loader, activation, dev)
    if batch_mode:
        return it
    out = [b['prob'] for b in it]
    return np.concatenate(out, axis=0) if out else np.zeros((0,))


__all__ = ['infer', 'apply_activation', 'load_model']
