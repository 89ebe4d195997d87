"""Native BERT fine-tuning step (the BASELINE "BERT-base fine-tune DAG" config).

embeddings+LN -> N native encoder layers -> pooler/classifier/softmax-CE -> backward
(weights' gradients straight into the flat arena, RCCL buckets all-reduced on the side
stream as they complete) -> fused AdamW per arena.  Captured into one HIP graph after
``warmup_eager`` eager steps, like the ResNet step; the dropout seed is a device scalar
advanced inside the graph.

Packed mode (``pack_tokens=T``): instead of a padded ``[batch, seq_len]`` rectangle the step
holds ``T`` token rows of whole sequences laid back to back, at most ``batch`` (``nseq_max``)
of them, each at most ``seq_len`` (``max_len``) long; attention runs the varlen kernels over
``cu_seqlens`` and no layer spends work on padding.  ``load_batch`` packs the usual padded
batch on the host; everything that varies per batch is device memory copied into outside the
graph, so one captured graph replays on any number and mix of lengths.  With ``world_size >
1`` each rank normalises its loss by its own number of sequences and the gradients are
averaged over ranks - what torch DDP does with uneven per-rank batches.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from mlcomp_amd.models import build_model
from mlcomp_amd.models.native_bert import NativeBert
from mlcomp_amd.parallel.comm import make_comm
from mlcomp_amd.parallel.ddp import GradBucketer
from mlcomp_amd.train.graphed import GraphedStep
from mlcomp_amd.train.optim import FusedAdam, FusedSGD


class NativeBertStep(GraphedStep):
    def __init__(self, model_name='bert-base', batch=32, seq_len=128, device=None, world_size=1, use_graph=True,
                 num_labels=2, lr=2e-5, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-6, seed=0, warmup_eager=2,
                 torch_model=None, dropout: Optional[float] = None, comm=None, optimizer='AdamW',
                 momentum=0.0, nesterov=False, dampening=0.0, pack_tokens: Optional[int] = None):
        self.device = torch.device(device or 'cuda')
        torch.manual_seed(seed)
        kw = {'num_labels': num_labels}
        if dropout is not None:
            kw.update(hidden_dropout=dropout, attention_dropout=dropout)
        tm = torch_model if torch_model is not None else build_model(model_name, **kw)
        self.packed = pack_tokens is not None
        self.net = NativeBert(tm, self.device, batch, seq_len, packed_tokens=pack_tokens)
        self.net.ctx.grad_prezeroed = True
        self.world = world_size
        self.comm = comm if comm is not None else (make_comm(self.device) if world_size > 1 else None)
        self.bucketer = GradBucketer(self.net.arena, self.comm)
        self.bucketer.broadcast_params()
        if optimizer in ('Adam', 'AdamW'):
            self.opt = FusedAdam(self.net.arena, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                 decoupled=optimizer == 'AdamW', grad_scale=1.0 / world_size)
        elif optimizer == 'SGD':
            self.opt = FusedSGD(self.net.arena, lr=lr, momentum=momentum, weight_decay=weight_decay,
                                nesterov=nesterov, dampening=dampening, grad_scale=1.0 / world_size)
        else:
            raise ValueError(f'native optimizers: SGD / Adam / AdamW, not {optimizer!r}')
        # optimizer-in-backward (MLC_OPT_IN_BWD=1): each gradient bucket is updated on the side
        # stream as soon as it is complete (and all-reduced).  Measured slower on MI355X
        # (profiles/round2_ab): the memory-bound update competes with the memory-bound
        # backward passes, so the default is one update launch per arena after backward.
        self.opt_in_bwd = os.environ.get('MLC_OPT_IN_BWD', '0') == '1'
        if self.opt_in_bwd:
            self.bucketer.attach_optimizer(self.opt)
        self.batch, self.seq_len = batch, seq_len
        rank = int(os.environ.get('RANK', '0'))
        g = torch.Generator(device=self.device)
        g.manual_seed(4321 + rank)
        c = self.net.c
        self.key_bias = None
        if self.packed:
            T = self.net.T
            self.ids = torch.zeros(T, dtype=torch.long, device=self.device)
            self.tt = torch.zeros(T, dtype=torch.long, device=self.device)
            self.y = torch.zeros(batch, dtype=torch.long, device=self.device)
            self.nseq = 0
            self._load_synthetic(num_labels, 4321 + rank)
        else:
            self.ids = torch.randint(0, c.vocab_size, (batch, seq_len), device=self.device, generator=g)
            self.tt = torch.zeros(batch, seq_len, dtype=torch.long, device=self.device)
            self.tt[:, seq_len // 2:] = 1
            self.y = torch.randint(0, num_labels, (batch,), device=self.device, generator=g)
        self.net.seed.fill_(seed * 7919 + rank)
        self.use_graph = use_graph and self.device.type == 'cuda'
        self.warmup_eager = warmup_eager
        self.graph = None
        self.calls = 0

    def _check_ids(self, ids):
        """Token ids past the vocabulary would make the embedding gather read out of bounds
        on the GPU (a device fault): refuse them while they are still on the host."""
        v = self.net.c.vocab_size
        if ids.device.type == 'cpu' and ids.numel() and (int(ids.max()) >= v or int(ids.min()) < 0):
            raise ValueError(f'token ids must be in [0, {v}) for this model (got [{int(ids.min())}, {int(ids.max())}])')

    # ------------------------------------------------------------------ packed mode
    def _load_synthetic(self, num_labels, seed):
        """A seeded batch of random lengths in [1, max_len] that fills the token budget, so a
        packed step runs before any real batch is loaded."""
        g = torch.Generator().manual_seed(seed)
        lens, total = [], 0
        while len(lens) < self.batch:
            n = int(torch.randint(1, self.seq_len + 1, (1,), generator=g))
            if total + n > self.net.T:
                break
            lens.append(n)
            total += n
        lens = lens or [min(self.seq_len, self.net.T)]
        n = len(lens)
        ids = torch.randint(0, self.net.c.vocab_size, (n, self.seq_len), generator=g)
        mask = (torch.arange(self.seq_len)[None] < torch.tensor(lens)[:, None]).long()
        tt = (torch.arange(self.seq_len)[None] >= torch.tensor(lens)[:, None] // 2).long() * mask
        self.load_batch(ids, torch.randint(0, num_labels, (n,), generator=g), tt, mask)

    def pack(self, ids, token_type_ids=None, attention_mask=None, nseq_max=None, tokens=None):
        """A padded ``[n, S]`` batch with a right-padding ``attention_mask`` -> the packed host
        tensors ``(ids [T], tt [T], pos_ids [T], cu_seqlens int32 [nseq_max + 1], lengths)``.
        ``nseq_max`` / ``tokens`` default to the engine's; ValueError when the batch has more
        sequences, more tokens or a longer sequence than the engine holds, or when the mask is
        not right-padded (ones, then zeros; at least one token)."""
        nseq_max = self.batch if nseq_max is None else nseq_max
        T = self.net.T if tokens is None else tokens
        ids = ids.cpu()
        n, S = ids.shape
        mask = torch.ones(n, S, dtype=torch.long) if attention_mask is None else attention_mask.cpu().long()
        lens = mask.sum(1)
        if not torch.equal(mask, (torch.arange(S)[None] < lens[:, None]).long()) or int(lens.min()) < 1:
            raise ValueError('packed mode needs a right-padded attention_mask: ones for the tokens of each '
                             'sequence (at least one), then zeros')
        if n > nseq_max:
            raise ValueError(f'{n} sequences in the batch, the packed engine holds nseq_max = {nseq_max}')
        if int(lens.max()) > self.seq_len:
            raise ValueError(f'a sequence of {int(lens.max())} tokens is over max_len = {self.seq_len}')
        total = int(lens.sum())
        if total > T:
            raise ValueError(f'{total} tokens in the batch, over the token budget pack_tokens = {T}')
        keep = mask.bool()
        tt = torch.zeros_like(ids) if token_type_ids is None else token_type_ids.cpu()
        out_ids, out_tt, pos = (torch.zeros(T, dtype=torch.long) for _ in range(3))
        out_ids[:total] = ids[keep]
        out_tt[:total] = tt[keep]
        pos[:total] = torch.arange(S)[None].expand(n, S)[keep]
        cu = torch.full((nseq_max + 1,), total, dtype=torch.int32)
        cu[0] = 0
        cu[1:n + 1] = torch.cumsum(lens, 0).to(torch.int32)
        return out_ids, out_tt, pos, cu, lens

    def load_packed(self, ids, labels, cu_seqlens, token_type_ids=None, pos_ids=None):
        """A batch that is already packed (a loader that packs itself): ``ids`` (and
        ``token_type_ids`` / ``pos_ids``) of up to T rows - missing tail rows are filled with 0 -
        ``cu_seqlens`` of up to nseq_max + 1 entries (missing slots are empty) and one label per
        given slot.  Slots of length 0 are empty: no loss, no gradient.  ``pos_ids`` defaults to
        the position within each sequence."""
        if not self.packed:
            raise RuntimeError('load_packed needs a step built with pack_tokens')
        T, nmax = self.net.T, self.batch
        self._check_ids(ids)
        cu_in = cu_seqlens.cpu().to(torch.int32)
        if ids.dim() != 1 or ids.numel() > T or cu_in.numel() > nmax + 1:
            raise ValueError(f'packed ids must be one row of at most {T} tokens with at most {nmax} sequences '
                             f'(got {tuple(ids.shape)}, {cu_in.numel() - 1} sequences)')
        from mlcomp_amd.ops.transformer import check_cu_seqlens
        check_cu_seqlens(cu_in, ids.numel(), self.seq_len)
        ns = cu_in.numel() - 1
        cu = torch.full((nmax + 1,), int(cu_in[-1]), dtype=torch.int32)
        cu[:ns + 1] = cu_in
        lens = (cu[1:] - cu[:-1]).long()
        nreal = int((lens > 0).sum())
        if nreal < 1:
            raise ValueError('a packed batch needs at least one sequence')
        if pos_ids is None:
            pos_ids = torch.arange(int(cu[-1])) - torch.repeat_interleave(cu[:-1].long(), lens)
        w = (lens > 0).float() / nreal
        y = torch.zeros(nmax, dtype=torch.long)
        y[:ns] = labels.cpu()[:ns]

        def rows(t):
            out = torch.zeros(T, dtype=torch.long)
            if t is not None:
                out[:t.numel()] = t.cpu()
            return out
        for dst, src in ((self.ids, rows(ids)), (self.tt, rows(token_type_ids)), (self.net.pos_ids, rows(pos_ids)),
                         (self.net.cu, cu), (self.y, y), (self.net.slot_w, w)):
            dst.copy_(src.to(self.device, non_blocking=True))
        self.nseq = nreal

    def load_text_batch(self, pb):
        """A batch staged by ``TextRecordLoader(layout='packed')`` (a ``PackedTextBatch``): one
        kernel writes the step's six static buffers from the staged slot, so it works before
        and after graph capture and nothing is packed on the host.  The batch must have been
        built for this step's token rows, slots and longest sequence."""
        if not self.packed:
            raise RuntimeError('load_text_batch needs a step built with pack_tokens')
        T, nmax = self.net.T, self.batch
        if (pb.T, pb.nmax, pb.max_len) != (T, nmax, self.seq_len):
            raise ValueError(f'the text batch was built for {pb.T} token rows, {pb.nmax} sequences of up to '
                             f'{pb.max_len} tokens; this step holds {T}, {nmax} and {self.seq_len}')
        c = self.net.c
        if pb.vocab > c.vocab_size or pb.num_labels > c.num_labels:
            raise ValueError(f'the text batch allows token ids below {pb.vocab} and labels below {pb.num_labels}; '
                             f'the model has vocab_size = {c.vocab_size} and {c.num_labels} labels')
        if pb.nseq < 1:
            raise ValueError('a packed batch needs at least one sequence')
        pb.unpack_into(self.ids, self.tt, self.net.pos_ids, self.net.cu, self.y, self.net.slot_w)
        self.nseq = pb.nseq

    def load_batch(self, ids, labels, token_type_ids=None, attention_mask=None):
        self._check_ids(ids)
        if self.packed:
            p_ids, p_tt, pos, cu, lens = self.pack(ids, token_type_ids, attention_mask)
            self.load_packed(p_ids[:int(cu[-1])], labels, cu[:lens.numel() + 1], p_tt, pos)
            return
        self.ids.copy_(ids.to(self.device, non_blocking=True))
        self.y.copy_(labels.to(self.device, non_blocking=True))
        if token_type_ids is not None:
            self.tt.copy_(token_type_ids.to(self.device, non_blocking=True))
        if attention_mask is not None:
            kb = torch.zeros(attention_mask.shape, device=self.device).masked_fill(
                attention_mask.to(self.device) == 0, float('-inf'))
            if self.key_bias is None:
                if self.graph is not None:
                    raise RuntimeError('attention masks must be enabled before the graph is captured')
                self.key_bias = kb
            else:
                self.key_bias.copy_(kb)

    def predict(self, ids, token_type_ids=None, attention_mask=None):
        """Native inference logits [B, num_labels] for one (eval) batch."""
        self._check_ids(ids)
        if self.packed:
            # packed the same way, at this batch's own size (nothing here is captured): the token
            # count rounded up to the GEMMs' multiple of 8, one slot per sequence
            total = int(attention_mask.sum()) if attention_mask is not None else ids.numel()
            p_ids, p_tt, pos, cu, _ = self.pack(ids, token_type_ids, attention_mask, nseq_max=ids.shape[0],
                                                tokens=(max(total, 1) + 7) // 8 * 8)
            dev = lambda t: t.to(self.device)  # noqa: E731
            return self.net.predict_packed(dev(p_ids), dev(p_tt), dev(pos), dev(cu), self.seq_len)
        ids = ids.to(self.device)
        tt = token_type_ids.to(self.device) if token_type_ids is not None else torch.zeros_like(ids)
        kb = None
        if attention_mask is not None:
            kb = torch.zeros(attention_mask.shape, device=self.device).masked_fill(
                attention_mask.to(self.device) == 0, float('-inf'))
        return self.net.predict(ids, tt, kb)

    def _body(self):
        net = self.net
        net.ctx.ws.zero()
        net.arena.zero_grad()
        net.seed.add_(1)
        self.bucketer.begin()
        loss = net.loss(self.ids, self.tt, self.key_bias, self.y)
        loss.backward()
        self.bucketer.finish()
        if not self.opt_in_bwd:
            self.opt.step()

    def set_lr(self, lr):
        self.opt.set_lr(lr)

    def samples(self) -> int:
        """Sequences the loaded batch trains on: the real ones in packed mode."""
        return self.nseq if self.packed else self.batch

    def last_loss(self) -> float:
        return float(self.net.loss_sum().item()) / self.samples()

    def accuracy(self) -> float:
        return float(self.net.correct().item()) / self.samples()


__all__ = ['NativeBertStep']
