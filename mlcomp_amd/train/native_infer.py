"""Native inference engine for the ResNet-family classifiers.

``NativeInference(torch_model, batch, image_size)`` lowers the model onto the native layers
(:class:`~mlcomp_amd.models.native_resnet.NativeResNet`), switches them to deploy mode -
every conv-BN(-add)(-ReLU) unit is ONE conv whose weights and bias carry the BatchNorm
(``ConvBN.refold``) and whose epilogue adds the shortcut and applies the ReLU
(``Fn.conv2d_fwd_res``) - and captures the whole forward into one HIP graph over a static
input and a static logits buffer.  Nothing in it goes to MIOpen or hipBLASLt.

``predict(x)`` takes any ``n <= batch`` rows: a short batch is copied into the front of the
static input, the rows behind it keep whatever the previous call left there, and the first
``n`` logits come back.  Inference BatchNorm makes rows independent, so the stale rows
cannot reach them.

Not folded: the space-to-depth stem (its own conv kernel plus the BN-apply pass, one unit).
"""
from __future__ import annotations

from typing import Optional

import torch

from mlcomp_amd.models.native_resnet import STEM_CIN, NativeResNet
from mlcomp_amd.ops import functional as Fn
from mlcomp_amd.train.graphed import GraphedStep, work_stream
from mlcomp_amd.train.native_spec import NativeUnsupported

NO_DEVICE = 'no HIP device: the native engines run on MI355X GPUs'


def unsupported_reason(model) -> Optional[str]:
    """None when the inference engine takes ``model``, else the reason it does not."""
    from mlcomp_amd.models.resnet import ResNet
    if not isinstance(model, torch.nn.Module):
        return (f'{type(model).__name__} is not an nn.Module (a TorchScript file cannot be lowered: pass the '
                'module, or a checkpoint plus a model spec)')
    if isinstance(model, torch.jit.ScriptModule):
        return 'a TorchScript module cannot be lowered: pass the nn.Module, or a checkpoint plus a model spec'
    if not isinstance(model, ResNet):
        return f'{type(model).__name__} has no native inference lowering (ResNet-family classifiers only)'
    if model.groups != 1:
        return f'ResNet with groups={model.groups}: the native convs are dense (groups=1)'
    if not model.include_top:
        return 'ResNet without its classifier head (include_top=False)'
    return None


class NativeInference(GraphedStep):
    warmup_eager = 1

    def __init__(self, torch_model, batch: int, image_size, device=None, use_graph: bool = True):
        reason = unsupported_reason(torch_model)
        if reason is not None:
            raise NativeUnsupported(reason)
        self.device = torch.device(device or ('cuda' if torch.cuda.is_available() else 'cpu'))
        self.torch_model = torch_model
        self.net = NativeResNet(torch_model, self.device)
        self.net.ctx.deploy = True
        self.net.eval()
        self.refold()
        H, W = (image_size, image_size) if isinstance(image_size, int) else tuple(image_size)
        self.batch = int(batch)
        self.classes = self.net.head.O
        self.x = self._prep(torch.zeros(self.batch, H, W, STEM_CIN, device=self.device, dtype=torch.bfloat16))
        self.out = torch.zeros(self.batch, self.classes, device=self.device, dtype=torch.float32)
        self.use_graph = bool(use_graph) and self.device.type == 'cuda'
        self.graph = None
        self.calls = 0

    # ------------------------------------------------------------------ weights
    def refold(self):
        """Fold every unit's BatchNorm into its conv again (after the weights changed)."""
        for u in self.net._units():
            u.refold()

    def load_state_dict(self, state_dict):
        """Weights in the PyTorch layout of the model (a training checkpoint's
        ``model_state_dict``).  The captured graph is dropped: the units re-create their
        statistics buffers, so the next ``predict`` warms up and captures again."""
        self.torch_model.load_state_dict(state_dict.get('model_state_dict', state_dict))
        self.graph = None
        self.calls = 0
        for u in self.net._units():
            u.load_from_torch()
        self.net.head.load_from_torch()
        self.net.ctx.arena.decay.refresh_mirror()
        self.refold()

    @classmethod
    def from_checkpoint(cls, path: str, model_spec: dict, batch: int, image_size, device=None,
                        use_graph: bool = True):
        """Build ``model_spec`` (``build_model`` keyword arguments, ``name`` first) and load the
        checkpoint the train executor wrote (``model_state_dict`` inside, or a bare one)."""
        from mlcomp_amd.models import build_model
        spec = dict(model_spec)
        model = build_model(spec.pop('name'), **spec)
        ck = torch.load(path, map_location='cpu', weights_only=True)
        model.load_state_dict(ck.get('model_state_dict', ck))
        return cls(model, batch, image_size, device=device, use_graph=use_graph)

    # ------------------------------------------------------------------ forward
    def _prep(self, x_nhwc):
        if getattr(self.net.stem, 's2d', False) and x_nhwc.shape[-1] != 16:
            return Fn.stem_s2d(x_nhwc, 3)
        return x_nhwc

    def _body(self):
        with torch.no_grad():
            self.out.copy_(self.net.logits(self.x))

    def predict(self, x: torch.Tensor) -> torch.Tensor:
        """fp32 logits [n, classes] of ``x``: NCHW float or NHWC bf16 (channels padded to the
        stem's 8), ``n <= batch`` rows."""
        n = x.shape[0]
        if not 1 <= n <= self.batch:
            raise ValueError(f'predict takes 1..{self.batch} rows, not {n}')
        with torch.no_grad(), work_stream(self.device):
            if x.dim() == 4 and x.shape[1] in (1, 3) and x.dtype != torch.bfloat16:
                x = Fn.nchw_to_nhwc(x.to(self.device, non_blocking=True).float(), pad_to=STEM_CIN)
            xp = self._prep(x.to(self.device, non_blocking=True))
            if tuple(xp.shape[1:]) != tuple(self.x.shape[1:]):
                raise ValueError(f'input rows of shape {tuple(xp.shape[1:])}, the engine was built for '
                                 f'{tuple(self.x.shape[1:])}')
            self.x[:n].copy_(xp)
            self.calls += 1
            self._call()
            return self.out[:n].clone()


__all__ = ['NativeInference', 'unsupported_reason', 'NO_DEVICE']
