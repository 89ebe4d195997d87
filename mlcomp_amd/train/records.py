"""Record files and the native input pipeline.

The reference trains from a PyTorch ``DataLoader`` over python datasets
(`mlcomp/contrib/dataset/classify.py:16-138`, driven by Catalyst).  On MI355X a step takes
~22 ms for 256 ImageNet images, so one node consumes ~92k images/s: the input pipeline is
split between the host and the GPU instead.

* ``.mlrec`` record file: fixed-size uint8 HWC images + int32 labels behind a 64-byte
  header (:func:`write_records`, :func:`pack_images`), memory-mapped by the C++ runtime
  (``csrc/runtime/records.cpp`` -> ``libmlcomp_runtime.so``).
* :class:`RecordLoader`: C++ worker threads copy the raw records of each batch into pinned
  ring slots and draw the per-sample augmentation (RandomResizedCrop box + flip, or the
  centre crop) from a counter-based RNG keyed by (seed, epoch, sample), so the stream is
  identical for any thread count.  Epochs are shuffled globally and sharded by rank.
  The uint8 batch crosses PCIe on a copy stream; one HIP kernel (``mlc_augment``,
  ``csrc/kernels/augment.hip``) crops, resizes, flips, normalises and writes the layout
  the model reads (the native ResNet stem's space-to-depth image, NHWC8 or NCHW fp32).
* :func:`augment_reference` is the same transform in PyTorch (CPU path, test oracle).
* Segmentation: ``MLSEG001`` files pair every image with a uint8 mask
  (:func:`write_seg_records`, :func:`pack_seg_images`, :class:`SegRecordFile`).
  :class:`SegRecordLoader` runs the same ring over them; the host draws the crop box plus
  hflip / vflip / transpose coins (the eight symmetries of the square) and one kernel
  (``mlc_augment_seg``) samples the image bilinearly and the mask by nearest neighbour at
  the same source coordinate.  :func:`augment_seg_reference` is its PyTorch twin.
* Video: ``MLVID001`` files hold clips of F uint8 frames and an int32 label
  (:func:`write_clip_records`, :func:`pack_clip_frames`, :class:`ClipRecordFile`).
  :class:`ClipRecordLoader` runs the same ring over them: the host draws one box and flip per
  clip (the classification draws) and the first frame ``t0``, copies only the ``clip_len``
  frames ``t0 + k*frame_stride`` into the slot, and one kernel (``mlc_augment_clip``)
  applies the transform to every frame and writes NCTHW fp32 or channels_last_3d bf16.
  :func:`augment_clip_reference` is its PyTorch twin.
* Text: ``MLTXT001`` files hold token sequences of different lengths behind an index
  (:func:`write_text_records`, :func:`pack_text_csv`, :class:`TextRecordFile`).
  :class:`TextRecordLoader` plans token-budget batches in C++ (the rule of
  ``TokenBudgetBatchSampler``), gathers each into one pinned int32 slot that crosses PCIe in
  one copy, and one kernel (``mlc_text_unpack``) writes every tensor the packed or padded
  BERT step reads.  :func:`text_unpack_reference` is its PyTorch twin.
"""
from __future__ import annotations

import ctypes as C
import itertools
import math
import weakref
import os
import struct
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

MAGIC = b'MLREC001'
HEADER = struct.Struct('<8s4I2Q24x')
SEG_MAGIC = b'MLSEG001'
SEG_HEADER = struct.Struct('<8s4I2Q2I16x')   # ... count, record_bytes, K, kind
MASK_KINDS = {'planes': 0, 'index': 1}
CLIP_MAGIC = b'MLVID001'
CLIP_HEADER = struct.Struct('<8s4I2QI20x')   # ... count, record_bytes, F (frames per record)
TEXT_MAGIC = b'MLTXT001'
TEXT_HEADER = struct.Struct('<8s4I2QQ16x')   # ... count, record_bytes (0), total_tokens
TEXT_ENTRY = np.dtype([('token_offset', '<u8'), ('length', '<u4'), ('type0_length', '<u4'), ('label', '<i4'),
                       ('zero', '<u4')])
TEXT_LAYOUTS = {'packed': 0, 'padded': 1}
LAYOUTS = {'s2d': 0, 'nhwc8': 1, 'nchw': 2}
CLIP_LAYOUTS = {'ncthw': 0, 'nthwc': 1}
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


# ------------------------------------------------------------------------- files
def write_records(path: str, images: Iterable, labels: Optional[Iterable[int]] = None,
                  shape: Optional[Tuple[int, int, int]] = None) -> int:
    """Write ``images`` (uint8 HWC arrays of one shape, or one [N, H, W, C] array) and their
    int labels to ``path``; returns the record count.  Written to ``path + '.tmp'`` and
    renamed, so a reader never sees a partial file."""
    if isinstance(images, np.ndarray) and images.ndim == 4:
        shape = images.shape[1:]
    it = iter(images)
    first = None
    if shape is None:
        first = np.asarray(next(it), dtype=np.uint8)
        shape = first.shape
    H, W, Cc = (int(s) for s in shape)
    rec_bytes = H * W * Cc + 4
    labs = iter(labels) if labels is not None else None
    tmp = path + '.tmp'
    n = 0
    with open(tmp, 'wb') as f:
        f.write(HEADER.pack(MAGIC, H, W, Cc, 4, 0, rec_bytes))

        def put(img):
            nonlocal n
            a = np.ascontiguousarray(img, dtype=np.uint8)
            if a.shape != (H, W, Cc):
                raise ValueError(f'record {n}: shape {a.shape} != {(H, W, Cc)}')
            f.write(a.tobytes())
            f.write(struct.pack('<i', int(next(labs)) if labs is not None else 0))
            n += 1
        if first is not None:
            put(first)
        for img in it:
            put(img)
        f.seek(0)
        f.write(HEADER.pack(MAGIC, H, W, Cc, 4, n, rec_bytes))
    os.replace(tmp, path)
    return n


def pack_images(paths: Sequence[str], labels: Sequence[int], out: str, size: int = 256) -> int:
    """Decode image files (PIL), resize the shorter side to ``size``, centre-crop a
    ``size`` x ``size`` square and write them as a record file."""
    from PIL import Image

    def gen():
        for p in paths:
            im = Image.open(p).convert('RGB')
            w, h = im.size
            s = size / min(w, h)
            im = im.resize((max(size, round(w * s)), max(size, round(h * s))), Image.BILINEAR)
            w, h = im.size
            l, t = (w - size) // 2, (h - size) // 2
            yield np.asarray(im.crop((l, t, l + size, t + size)), dtype=np.uint8)
    return write_records(out, gen(), labels, shape=(size, size, 3))


class RecordFile:
    """numpy view of a record file (header checks, random access) - the python twin of the
    C++ reader, used by tests and tools."""

    def __init__(self, path: str):
        with open(path, 'rb') as f:
            magic, H, W, Cc, lb, n, rb = HEADER.unpack(f.read(HEADER.size))
        if magic != MAGIC or lb != 4 or rb != H * W * Cc + 4:
            raise ValueError(f'{path}: not an mlrec file')
        self.shape = (H, W, Cc)
        self.count = n
        self._m = np.memmap(path, dtype=np.uint8, mode='r', offset=HEADER.size, shape=(n, rb))

    def __len__(self):
        return self.count

    def image(self, i: int) -> np.ndarray:
        H, W, Cc = self.shape
        return np.asarray(self._m[i, :H * W * Cc]).reshape(H, W, Cc)

    def label(self, i: int) -> int:
        return int(np.asarray(self._m[i, -4:]).view('<i4')[0])


def write_seg_records(path: str, images: Iterable, masks: Iterable, kind: str = 'planes') -> int:
    """Write uint8 HWC ``images`` and their uint8 ``masks`` ([H, W, K] or [H, W]) to an
    image + mask record file; returns the record count.  ``kind='planes'``: K = 1..4 binary
    planes, a pixel is foreground for plane k iff its byte is non-zero; ``kind='index'``:
    K = 1, the byte is the class id.  Written to ``path + '.tmp'`` and renamed."""
    if kind not in MASK_KINDS:
        raise ValueError(f'mask kind: planes / index, not {kind!r}')
    it, mit = iter(images), iter(masks)
    tmp = path + '.tmp'
    n = 0
    H = W = Cc = K = None

    def header(count):
        return SEG_HEADER.pack(SEG_MAGIC, H, W, Cc, H * W * K, count, H * W * (Cc + K), K, MASK_KINDS[kind])
    try:
        with open(tmp, 'wb') as f:
            for img, m in zip(it, mit):
                a = np.ascontiguousarray(img, dtype=np.uint8)
                m = np.ascontiguousarray(m, dtype=np.uint8)
                if m.ndim == 2:
                    m = m[:, :, None]
                if H is None:
                    (H, W, Cc), K = a.shape, m.shape[2]
                if n == 0:
                    if not (1 <= Cc <= 4 and 1 <= K <= 4) or (kind == 'index' and K != 1):
                        raise ValueError(f'{Cc} image channels / {K} {kind} mask planes: 1..4 each, index masks 1')
                    f.write(header(0))
                if a.shape != (H, W, Cc) or m.shape != (H, W, K):
                    raise ValueError(f'record {n}: shapes {a.shape} / {m.shape} != {(H, W, Cc)} / {(H, W, K)}')
                f.write(a.tobytes())
                f.write(m.tobytes())
                n += 1
            if n == 0:
                raise ValueError('no records')
            f.seek(0)
            f.write(header(n))
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    os.replace(tmp, path)
    return n


def pack_seg_images(image_paths: Sequence[str], mask_paths: Sequence[str], out: str, size: int = 256,
                    kind: str = 'planes') -> int:
    """Decode image / mask file pairs (PIL) into an image + mask record file: the image's
    shorter side is resized to ``size`` (bilinear) and a ``size`` x ``size`` square is
    centre-cropped; the mask gets the same geometry with nearest resampling.  Masks are
    read as one 8-bit plane ('L'; palette files keep their indices)."""
    from PIL import Image
    if len(image_paths) != len(mask_paths):
        raise ValueError(f'{len(image_paths)} images but {len(mask_paths)} masks')

    def fit(im, resample):
        w, h = im.size
        s = size / min(w, h)
        im = im.resize((max(size, round(w * s)), max(size, round(h * s))), resample)
        w, h = im.size
        l, t = (w - size) // 2, (h - size) // 2
        return np.asarray(im.crop((l, t, l + size, t + size)), dtype=np.uint8)

    def pairs():
        for ip, mp in zip(image_paths, mask_paths):
            im, m = Image.open(ip).convert('RGB'), Image.open(mp)
            if m.mode not in ('L', 'P'):
                m = m.convert('L')
            if im.size != m.size:
                raise ValueError(f'{ip}: image {im.size} and mask {m.size} differ in size')
            yield fit(im, Image.BILINEAR), fit(m, Image.NEAREST)
    # zip() in the writer draws from the two branches in turn, so tee holds one pair at most
    a, b = itertools.tee(pairs())
    return write_seg_records(out, (p[0] for p in a), (p[1] for p in b), kind=kind)


class SegRecordFile:
    """numpy view of an image + mask record file (the python twin of ``mlr_seg_open``)."""

    def __init__(self, path: str):
        with open(path, 'rb') as f:
            raw = f.read(SEG_HEADER.size)
        if len(raw) < SEG_HEADER.size:
            raise ValueError(f'{path}: not an image + mask mlrec file')
        magic, H, W, Cc, lb, n, rb, K, kind = SEG_HEADER.unpack(raw)
        if magic != SEG_MAGIC or not 1 <= K <= 4 or kind > 1 or (kind == 1 and K != 1) or not 1 <= Cc <= 4 \
                or lb != H * W * K or rb != H * W * (Cc + K):
            raise ValueError(f'{path}: not an image + mask mlrec file')
        self.shape = (H, W, Cc)
        self.planes = K
        self.kind = 'index' if kind else 'planes'
        self.count = n
        self._m = np.memmap(path, dtype=np.uint8, mode='r', offset=SEG_HEADER.size, shape=(n, rb))

    def __len__(self):
        return self.count

    def image(self, i: int) -> np.ndarray:
        H, W, Cc = self.shape
        return np.asarray(self._m[i, :H * W * Cc]).reshape(H, W, Cc)

    def mask(self, i: int) -> np.ndarray:
        H, W, Cc = self.shape
        return np.asarray(self._m[i, H * W * Cc:]).reshape(H, W, self.planes)


def write_clip_records(path: str, clips: Iterable, labels: Iterable[int]) -> int:
    """Write uint8 ``clips`` ([F, H, W, C] arrays of one shape, or one [N, F, H, W, C] array;
    F >= 1, C = 1..4) and their int labels to a clip record file; returns the record count.
    Written to ``path + '.tmp'`` and renamed; the tmp file is removed on error."""
    tmp = path + '.tmp'
    n = 0
    shape = None
    labs = iter(labels)

    def header(count):
        F, H, W, Cc = shape
        return CLIP_HEADER.pack(CLIP_MAGIC, H, W, Cc, 4, count, F * H * W * Cc + 4, F)
    try:
        with open(tmp, 'wb') as f:
            for clip in clips:
                a = np.ascontiguousarray(clip, dtype=np.uint8)
                if shape is None:
                    if a.ndim != 4 or a.shape[0] < 1 or not 1 <= a.shape[3] <= 4:
                        raise ValueError(f'clip shape {a.shape}: [F, H, W, C] with F >= 1 and C = 1..4')
                    shape = tuple(int(v) for v in a.shape)
                    f.write(header(0))
                if a.shape != shape:
                    raise ValueError(f'record {n}: shape {a.shape} != {shape}')
                try:
                    lab = int(next(labs))
                except StopIteration:
                    raise ValueError(f'record {n}: more clips than labels') from None
                f.write(a.tobytes())
                f.write(struct.pack('<i', lab))
                n += 1
            if n == 0:
                raise ValueError('no records')
            f.seek(0)
            f.write(header(n))
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    os.replace(tmp, path)
    return n


def pack_clip_frames(video_dirs: Sequence[str], labels: Sequence[int], out: str, frames: int, size: int = 128,
                     frame_step: int = 1, pad_short: bool = False) -> int:
    """Pack folders of frame images (one folder per video, files sorted by name) into a clip
    record file of ``frames`` frames per record.  Frames ``off + i*frame_step`` are taken,
    the window centred in the folder; each is resized (shorter side to ``size``, bilinear)
    and centre-cropped to ``size`` x ``size`` as :func:`pack_images` does.  A folder with
    fewer than ``(frames-1)*frame_step + 1`` frames is an error that names it, unless
    ``pad_short`` repeats its last frame."""
    from PIL import Image
    if frames < 1 or frame_step < 1:
        raise ValueError(f'frames {frames} / frame_step {frame_step}: both >= 1')
    if len(video_dirs) != len(labels):
        raise ValueError(f'{len(video_dirs)} videos but {len(labels)} labels')
    span = (frames - 1) * frame_step + 1

    def fit(p):
        im = Image.open(p).convert('RGB')
        w, h = im.size
        s = size / min(w, h)
        im = im.resize((max(size, round(w * s)), max(size, round(h * s))), Image.BILINEAR)
        w, h = im.size
        l, t = (w - size) // 2, (h - size) // 2
        return np.asarray(im.crop((l, t, l + size, t + size)), dtype=np.uint8)

    def gen():
        for d in video_dirs:
            files = sorted(os.listdir(d))
            if not files or (len(files) < span and not pad_short):
                raise ValueError(f'{d}: {len(files)} frames, {span} needed '
                                 f'({frames} frames at step {frame_step})')
            off = max(0, (len(files) - span) // 2)
            idx = [min(off + i * frame_step, len(files) - 1) for i in range(frames)]
            yield np.stack([fit(os.path.join(d, files[j])) for j in idx])
    return write_clip_records(out, gen(), labels)


class ClipRecordFile:
    """numpy view of a clip record file (the python twin of ``mlr_clip_open``)."""

    def __init__(self, path: str):
        with open(path, 'rb') as f:
            raw = f.read(CLIP_HEADER.size)
        if len(raw) < CLIP_HEADER.size:
            raise ValueError(f'{path}: not a clip record file')
        magic, H, W, Cc, lb, n, rb, F = CLIP_HEADER.unpack(raw)
        if magic != CLIP_MAGIC or F < 1 or not 1 <= Cc <= 4 or lb != 4 or rb != F * H * W * Cc + 4:
            raise ValueError(f'{path}: not a clip record file')
        self.shape = (H, W, Cc)
        self.frames = F
        self.count = n
        self._m = np.memmap(path, dtype=np.uint8, mode='r', offset=CLIP_HEADER.size, shape=(n, rb))

    def __len__(self):
        return self.count

    def clip(self, i: int) -> np.ndarray:
        H, W, Cc = self.shape
        return np.asarray(self._m[i, :-4]).reshape(self.frames, H, W, Cc)

    def label(self, i: int) -> int:
        return int(np.asarray(self._m[i, -4:]).view('<i4')[0])


def write_text_records(path: str, sequences: Iterable, labels: Iterable[int], token_types: Optional[Iterable] = None,
                       vocab_size: Optional[int] = None, type0_lengths: Optional[Iterable[int]] = None) -> int:
    """Write token ``sequences`` (rows of ids in ``[0, vocab_size)``, at least one token each)
    and their int labels to a text record file; returns the record count.  Token types come
    as ``token_types`` (one row per sequence: zeros, then ones - anything else is refused) or
    as ``type0_lengths`` (how many leading tokens of each sequence have type 0); neither:
    all type 0.  Tokens are stored as u16 when the vocabulary fits, else u32.  Written to
    ``path + '.tmp'`` and renamed; the tmp file is removed on error."""
    if vocab_size is None or int(vocab_size) < 1:
        raise ValueError('write_text_records needs the vocab_size the ids were made for')
    vocab_size = int(vocab_size)
    if token_types is not None and type0_lengths is not None:
        raise ValueError('token_types or type0_lengths, not both')
    types = iter(token_types) if token_types is not None else None
    t0s = iter(type0_lengths) if type0_lengths is not None else None
    labs = iter(labels)
    rows, entries, off = [], [], 0
    for n, seq in enumerate(sequences):
        a = np.asarray(seq, dtype=np.int64).reshape(-1)
        if a.size < 1:
            raise ValueError(f'record {n}: an empty sequence')
        if int(a.min()) < 0 or int(a.max()) >= vocab_size:
            raise ValueError(f'record {n}: token ids must be in [0, {vocab_size}) '
                             f'(got [{int(a.min())}, {int(a.max())}])')
        t0 = a.size
        if types is not None:
            t = np.asarray(next(types), dtype=np.int64).reshape(-1)
            t0 = int((t == 0).sum())
            if t.size != a.size or not np.array_equal(t, (np.arange(a.size) >= t0).astype(np.int64)):
                raise ValueError(f'record {n}: token types must be zeros followed by ones, one per token')
        elif t0s is not None:
            t0 = int(next(t0s))
            if not 0 <= t0 <= a.size:
                raise ValueError(f'record {n}: type0_length {t0} outside [0, {a.size}]')
        try:
            lab = int(next(labs))
        except StopIteration:
            raise ValueError(f'record {n}: more sequences than labels') from None
        rows.append(a)
        entries.append((off, a.size, t0, lab, 0))
        off += a.size
    if not rows:
        raise ValueError('no records')
    tb = 2 if vocab_size <= 65536 else 4
    index = np.array(entries, dtype=TEXT_ENTRY)
    tmp = path + '.tmp'
    try:
        with open(tmp, 'wb') as f:
            f.write(TEXT_HEADER.pack(TEXT_MAGIC, int(index['length'].max()), vocab_size, tb, 4, len(rows), 0, off))
            f.write(index.tobytes())
            f.write(np.concatenate(rows).astype('<u2' if tb == 2 else '<u4').tobytes())
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    os.replace(tmp, path)
    return len(rows)


class TextRecordFile:
    """numpy view of a text record file (the python twin of ``mlr_text_open``, with its
    checks) and a map-style dataset: item i is the dict ``SyntheticTextClassification`` gives,
    right-padded to ``seq_len`` (default: the file's longest record; a shorter ``seq_len`` is
    refused, truncation happens at pack time)."""

    def __init__(self, path: str, seq_len: Optional[int] = None):
        size = os.path.getsize(path)
        with open(path, 'rb') as f:
            raw = f.read(TEXT_HEADER.size)
        bad = ValueError(f'{path}: not a text record file')
        if len(raw) < TEXT_HEADER.size:
            raise bad
        magic, H, V, tb, lb, n, rb, total = TEXT_HEADER.unpack(raw)
        if magic != TEXT_MAGIC or n < 1 or lb != 4 or rb != 0 or H < 1 or V < 1 \
                or not (tb == 4 or (tb == 2 and V <= 65536)):
            raise bad
        if size < TEXT_HEADER.size + n * TEXT_ENTRY.itemsize + total * tb:
            raise bad
        self.index = np.memmap(path, dtype=TEXT_ENTRY, mode='r', offset=TEXT_HEADER.size, shape=(n,))
        ln, off = self.index['length'].astype(np.int64), self.index['token_offset']
        if int(ln.min()) < 1 or int(ln.max()) > H or bool((self.index['type0_length'] > ln).any()) \
                or int(off.max()) > total or bool((ln > total - off.astype(np.int64)).any()):
            raise bad
        self.count, self.max_len, self.vocab_size, self.token_bytes, self.total_tokens = n, H, V, tb, total
        self.seq_len = H if seq_len is None else int(seq_len)
        if self.seq_len < H:
            raise ValueError(f'{path}: seq_len {self.seq_len} is shorter than the longest record ({H} tokens)')
        self._tok = np.memmap(path, dtype='<u2' if tb == 2 else '<u4', mode='r',
                              offset=TEXT_HEADER.size + n * TEXT_ENTRY.itemsize, shape=(total,))

    def __len__(self):
        return self.count

    def lengths(self):
        return self.index['length'].tolist()

    def tokens(self, i: int) -> np.ndarray:
        e = self.index[i]
        return np.asarray(self._tok[int(e['token_offset']):int(e['token_offset']) + int(e['length'])]).astype(np.int64)

    def label(self, i: int) -> int:
        return int(self.index[i]['label'])

    def type0_length(self, i: int) -> int:
        return int(self.index[i]['type0_length'])

    def __getitem__(self, i: int):
        t = self.tokens(i)
        S, n = self.seq_len, t.size
        ids = torch.zeros(S, dtype=torch.long)
        ids[:n] = torch.from_numpy(t)
        pos = torch.arange(S)
        mask = (pos < n).long()
        return {'input_ids': ids, 'token_type_ids': (pos >= self.type0_length(i)).long() * mask,
                'attention_mask': mask, 'targets': self.label(i)}


def pack_text_csv(csv_path: str, vocab_path: str, out: str, text_col: str = 'text', label_col: str = 'label',
                  text_b_col: Optional[str] = None, max_len: int = 128, lower: bool = True,
                  fold_csv: Optional[str] = None, fold: Optional[int] = None, exclude_fold: bool = False):
    """Tokenise the rows of a CSV with :class:`~mlcomp_amd.train.tokenizer.WordPieceTokenizer`
    (``[CLS] a [SEP]`` or, with ``text_b_col``, ``[CLS] a [SEP] b [SEP]``, truncated to
    ``max_len``) and write a text record file.  Labels are the sorted distinct values of
    ``label_col``; returns ``(records, label names)``.  ``fold_csv`` (a ``fold`` column, rows
    aligned with the CSV's) keeps the rows of ``fold`` only, or every other fold with
    ``exclude_fold``."""
    import pandas as pd
    from .tokenizer import WordPieceTokenizer
    df = pd.read_csv(csv_path)
    for col in (text_col, label_col) + ((text_b_col,) if text_b_col else ()):
        if col not in df.columns:
            raise ValueError(f'{csv_path}: no column {col!r} (has {", ".join(map(str, df.columns))})')
    names = sorted(df[label_col].astype(str).unique())
    if fold_csv:
        folds = pd.read_csv(fold_csv)
        if len(folds) != len(df) or 'fold' not in folds.columns:
            raise ValueError(f'{fold_csv}: needs a fold column with one row per row of {csv_path}')
        if fold is not None:
            keep = (folds['fold'] != fold) if exclude_fold else (folds['fold'] == fold)
            df = df[keep.values]
    elif fold is not None and 'fold' in df.columns:
        df = df[(df['fold'] != fold) if exclude_fold else (df['fold'] == fold)]
    tok = WordPieceTokenizer(vocab_path, lower=lower)
    seqs, t0s, labels = [], [], []
    for _, row in df.iterrows():
        b = None if not text_b_col or pd.isna(row[text_b_col]) else str(row[text_b_col])
        ids, t0 = tok.encode('' if pd.isna(row[text_col]) else str(row[text_col]), b, max_len=max_len)
        seqs.append(ids)
        t0s.append(t0)
        labels.append(names.index(str(row[label_col])))
    n = write_text_records(out, seqs, labels, type0_lengths=t0s, vocab_size=len(tok.vocab))
    return n, names


# ------------------------------------------------------------------------- runtime
_RT = None


def runtime():
    """ctypes handle of libmlcomp_runtime.so (built in-tree on first use)."""
    global _RT
    if _RT is not None:
        return _RT
    from mlcomp_amd.build import RUNTIME_LIB, build_runtime
    if not os.path.exists(RUNTIME_LIB):
        build_runtime()
    lib = C.CDLL(RUNTIME_LIB)
    vp, i32, i64, u64, f64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_double
    sig = {
        'mlr_open': ([C.c_char_p], vp), 'mlr_close': ([vp], None), 'mlr_shape': ([vp, vp], None),
        'mlr_loader_create': ([vp, i32, i32, i32, i32, f64, f64, f64, f64, u64, i32, i32, i32, i32, i32, i32], vp),
        'mlr_loader_set_slot': ([vp, i32, vp, vp, vp], i32),
        'mlr_loader_start_epoch': ([vp, u64], i64),
        'mlr_loader_next': ([vp, vp], i32), 'mlr_loader_release': ([vp, i32], None),
        'mlr_loader_destroy': ([vp], None),
        'mlr_seg_open': ([C.c_char_p], vp), 'mlr_seg_shape': ([vp, vp], None),
        'mlr_seg_loader_create': ([vp, i32, i32, i32, i32, f64, f64, f64, f64, u64, i32, i32, i32, i32, i32, i32],
                                  vp),
        'mlr_seg_loader_set_slot': ([vp, i32, vp, vp, vp], i32),
        'mlr_clip_open': ([C.c_char_p], vp), 'mlr_clip_shape': ([vp, vp], None),
        'mlr_clip_loader_create': ([vp, i32, i32, i32, i32, i32, i32, f64, f64, f64, f64, u64, i32, i32, i32, i32,
                                    i32, i32], vp),
        'mlr_clip_loader_set_slot': ([vp, i32, vp, vp, vp], i32),
        'mlr_text_open': ([C.c_char_p], vp), 'mlr_text_shape': ([vp, vp], None),
        'mlr_text_loader_create': ([vp, i32, i32, i32, i32, u64, i32, i32, i32, i32, i32], vp),
        'mlr_text_loader_set_slot': ([vp, i32, vp], i32),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, res
    _RT = lib
    return lib


def augment_reference(img: torch.Tensor, par: torch.Tensor, out_h: int, out_w: int, mean_istd: Sequence[float],
                      layout: str = 'nchw') -> torch.Tensor:
    """PyTorch twin of ``mlc_augment``: img uint8 [B, H, W, C], par int [B, 5]
    (y0, x0, h, w, flip) -> the normalised crops in ``layout``."""
    B, H, W, Cc = img.shape
    p = par.long()
    oy = torch.arange(out_h, dtype=torch.float32)
    ox = torch.arange(out_w, dtype=torch.float32)
    outs = []
    for b in range(B):
        y0, x0, h, w, flip = p[b].tolist()
        xs = (out_w - 1 - ox) if flip else ox
        fy = ((oy + 0.5) * (h / out_h) - 0.5).clamp(0, h - 1)
        fx = ((xs + 0.5) * (w / out_w) - 0.5).clamp(0, w - 1)
        iy0, ix0 = fy.floor().long(), fx.floor().long()
        iy1, ix1 = (iy0 + 1).clamp(max=h - 1), (ix0 + 1).clamp(max=w - 1)
        wy, wx = (fy - iy0)[:, None, None], (fx - ix0)[None, :, None]
        im = img[b].float()
        g = lambda yy, xx: im[y0 + yy][:, x0 + xx]  # noqa: E731
        top = g(iy0, ix0) + wx * (g(iy0, ix1) - g(iy0, ix0))
        bot = g(iy1, ix0) + wx * (g(iy1, ix1) - g(iy1, ix0))
        outs.append(top + wy * (bot - top))
    return _normalise(torch.stack(outs), mean_istd, layout)


def _normalise(x: torch.Tensor, mean_istd: Sequence[float], layout: str) -> torch.Tensor:
    """[B, oh, ow, C] samples in 0..255 -> (x - mean) / std in ``layout``."""
    Cc = x.shape[-1]
    mean = torch.tensor(mean_istd[:Cc])
    istd = torch.tensor(mean_istd[4:4 + Cc])
    x = (x - mean) * istd
    if layout == 'nchw':
        return x.permute(0, 3, 1, 2).contiguous()
    if layout == 'nhwc8':
        return torch.nn.functional.pad(x, (0, 8 - Cc)).to(torch.bfloat16)
    from mlcomp_amd.ops.functional import stem_s2d
    return stem_s2d(x.to(torch.bfloat16), 3)


def augment_seg_reference(img: torch.Tensor, mask: torch.Tensor, par: torch.Tensor, out_h: int, out_w: int,
                          mean_istd: Sequence[float], layout: str = 'nchw', mask_kind: str = 'planes'):
    """PyTorch twin of ``mlc_augment_seg``: img uint8 [B, H, W, C], mask uint8 [B, H, W, K],
    par int [B, 8] (y0, x0, h, w, hflip, vflip, transpose, 0) -> (images in ``layout``,
    masks: ``planes`` fp32 0/1 [B, oh, ow, K] in pixel order, ``index`` int64 [B, oh, ow]).

    Output pixel (oy, ox) reads the box at row u of gh and column v of gw, where
    (u, v, gh, gw) = (ox, oy, ow, oh) under transpose and (oy, ox, oh, ow) otherwise, then
    hflip: v = gw-1-v and vflip: u = gh-1-u.  The image is the bilinear sample of
    :func:`augment_reference` there; the mask is the nearest source pixel in integers,
    row ((2u+1)*h) // (2*gh), column ((2v+1)*w) // (2*gw)."""
    B, H, W, Cc = img.shape
    p = par.long()
    oy = torch.arange(out_h)[:, None].expand(out_h, out_w)
    ox = torch.arange(out_w)[None, :].expand(out_h, out_w)
    outs, mouts = [], []
    for b in range(B):
        y0, x0, h, w, hflip, vflip, tr = p[b, :7].tolist()
        y0, x0 = min(max(y0, 0), H - 1), min(max(x0, 0), W - 1)      # the kernel clamps the box
        h, w = min(max(h, 1), H - y0), min(max(w, 1), W - x0)        # into the image as well
        u, v, gh, gw = (ox, oy, out_w, out_h) if tr else (oy, ox, out_h, out_w)
        if hflip:
            v = gw - 1 - v
        if vflip:
            u = gh - 1 - u
        fy = ((u.float() + 0.5) * (h / gh) - 0.5).clamp(0, h - 1)
        fx = ((v.float() + 0.5) * (w / gw) - 0.5).clamp(0, w - 1)
        iy0, ix0 = fy.floor().long(), fx.floor().long()
        iy1, ix1 = (iy0 + 1).clamp(max=h - 1), (ix0 + 1).clamp(max=w - 1)
        wy, wx = (fy - iy0)[:, :, None], (fx - ix0)[:, :, None]
        im = img[b].float()
        g = lambda yy, xx: im[y0 + yy, x0 + xx]  # noqa: E731
        top = g(iy0, ix0) + wx * (g(iy0, ix1) - g(iy0, ix0))
        bot = g(iy1, ix0) + wx * (g(iy1, ix1) - g(iy1, ix0))
        outs.append(top + wy * (bot - top))
        row, col = ((2 * u + 1) * h) // (2 * gh), ((2 * v + 1) * w) // (2 * gw)
        mouts.append(mask[b][y0 + row, x0 + col])
    m = torch.stack(mouts)                                  # [B, oh, ow, K] uint8
    m = m[..., 0].long() if mask_kind == 'index' else (m != 0).float()
    return _normalise(torch.stack(outs), mean_istd, layout), m


def augment_clip_reference(clips: torch.Tensor, par: torch.Tensor, out_h: int, out_w: int,
                           mean_istd: Sequence[float], layout: str = 'ncthw') -> torch.Tensor:
    """PyTorch twin of ``mlc_augment_clip``: clips uint8 [B, T, H, W, C], par int [B, 8]
    (y0, x0, h, w, flip, t0, frame stride, 0; the last three are not read) -> the normalised
    clips, logical [B, C, T, oh, ow]: fp32 contiguous for ``ncthw``, bf16 in channels_last_3d
    storage ([B, T, oh, ow, C] in memory) for ``nthwc``.  Every frame is
    :func:`augment_reference` with the clip's box, clamped into the image as the kernel
    clamps it."""
    if layout not in CLIP_LAYOUTS:
        raise ValueError(f'clip layout: {" / ".join(CLIP_LAYOUTS)}, not {layout!r}')
    B, T, H, W, Cc = clips.shape
    p = par.long()[:, :5].clone()
    p[:, 0].clamp_(0, H - 1)
    p[:, 1].clamp_(0, W - 1)
    p[:, 2] = torch.minimum(p[:, 2].clamp(min=1), H - p[:, 0])
    p[:, 3] = torch.minimum(p[:, 3].clamp(min=1), W - p[:, 1])
    x = torch.stack([augment_reference(clips[:, t], p, out_h, out_w, mean_istd, 'nchw') for t in range(T)], dim=2)
    if layout == 'nthwc':
        return x.permute(0, 2, 3, 4, 1).contiguous().to(torch.bfloat16).permute(0, 4, 1, 2, 3)
    return x


class RecordLoader:
    """Batches of a record file: dicts {'features', 'targets'} on ``device``.

    ``train``: RandomResizedCrop(scale, ratio) + horizontal flip, reshuffled every epoch;
    otherwise the centre ``out_size`` crop in file order.  ``rank`` / ``world_size`` shard
    each epoch like a DistributedSampler (padding by wrap-around); ``drop_last`` (default:
    ``train``) drops a last partial batch, otherwise it is completed by wrapping.
    ``threads`` host workers, ``depth`` pinned ring slots (>= 3)."""

    PAR = 5   # ints per sample in a slot's params
    LAYOUT_NAMES = LAYOUTS

    def __init__(self, path: str, batch_size: int, out_size=224, train: bool = True,
                 scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), seed: int = 0, rank: int = 0, world_size: int = 1,
                 shuffle: Optional[bool] = None, drop_last: Optional[bool] = None, threads: int = 8,
                 depth: int = 4, layout: str = 's2d', mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None,
                 chunk: int = 16):
        self.path = path
        self.batch_size = int(batch_size)
        self.out_h, self.out_w = (int(v) for v in out_size) if isinstance(out_size, (tuple, list)) \
            else (int(out_size), int(out_size))
        self.train = bool(train)
        self.layout = layout
        self.device = torch.device(device or ('cuda' if torch.cuda.is_available() else 'cpu'))
        self.epoch = 0
        self._explicit_epoch = False
        rt = runtime()
        self._rt = rt
        self._open(path)
        if layout not in self.LAYOUT_NAMES or (layout == 's2d' and (self.C != 3 or self.out_h % 2 or self.out_w % 2)):
            raise ValueError(f'layout {layout!r} does not fit {self.C}-channel images of {out_size}')
        ms = [0.0] * 8
        for c in range(min(self.C, 4)):
            m, s = (mean[c], std[c]) if c < len(mean) else (0.0, 1.0)
            ms[c], ms[4 + c] = m * 255.0, 1.0 / (s * 255.0)
        self.mean_istd = ms
        shuffle = self.train if shuffle is None else shuffle
        drop_last = self.train if drop_last is None else drop_last
        per = math.ceil(self.count / world_size)
        self._per = per
        self._drop_last = bool(drop_last)
        self._live = None
        self._len = per // self.batch_size if drop_last else math.ceil(per / self.batch_size)
        self._loader = self._create(self._file, self.batch_size, self.out_h, self.out_w, int(self.train),
                                            float(scale[0]), float(scale[1]), float(ratio[0]), float(ratio[1]),
                                            int(seed), int(rank), int(world_size), int(shuffle), int(drop_last),
                                            int(threads), int(chunk))
        if not self._loader:
            raise ValueError('bad loader arguments')
        pin = self.device.type == 'cuda'
        B = self.batch_size
        self._slots = []
        for i in range(max(3, int(depth))):
            img = self._image_buffer(pin_memory=pin)
            lab = self._target_buffer(pin_memory=pin)
            par = torch.empty(B, self.PAR, dtype=torch.int32, pin_memory=pin)
            self._set_slot(self._loader, i, C.c_void_p(img.data_ptr()), C.c_void_p(lab.data_ptr()),
                           C.c_void_p(par.data_ptr()))
            self._slots.append((img, lab, par))
        if self.device.type == 'cuda':
            self._copy_stream = torch.cuda.Stream(self.device)
            self._dev = [self._staging() for _ in range(2)]
            self._ms_dev = torch.tensor(ms, dtype=torch.float32, device=self.device)
            self._used = [None, None]   # event: the augment kernel that last read each staging buffer

    # what a segmentation or clip loader does differently (SegRecordLoader, ClipRecordLoader)
    def _open(self, path):
        rt = self._rt
        self._file = rt.mlr_open(path.encode())
        if not self._file:
            raise ValueError(f'{path}: cannot open record file')
        shp = (C.c_uint64 * 4)()
        rt.mlr_shape(self._file, shp)
        self.count, self.H, self.W, self.C = (int(v) for v in shp)
        self._create, self._set_slot = rt.mlr_loader_create, rt.mlr_loader_set_slot

    def _image_buffer(self, **kw):
        return torch.empty(self.batch_size, self.H, self.W, self.C, dtype=torch.uint8, **kw)

    def _target_buffer(self, **kw):
        return torch.empty(self.batch_size, dtype=torch.int64, **kw)

    def _staging(self):
        return (self._image_buffer(device=self.device),
                torch.empty(self.batch_size, self.PAR, dtype=torch.int32, device=self.device))

    def _augment_cpu(self, slot):
        img, lab, par = slot
        return augment_reference(img, par, self.out_h, self.out_w, self.mean_istd, self.layout), lab.clone()

    # the sampler-like API the runner calls
    @property
    def sampler(self):
        return self

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)
        self._explicit_epoch = True

    def __len__(self):
        return self._len

    @property
    def dataset(self):
        return range(self.count)

    def _out_shape(self, B):
        if self.layout == 's2d':
            return (B, (self.out_h + 6) // 2, (self.out_w + 6) // 2, 16), torch.bfloat16
        if self.layout == 'nhwc8':
            return (B, self.out_h, self.out_w, 8), torch.bfloat16
        return (B, self.C, self.out_h, self.out_w), torch.float32

    def _augment_gpu(self, k, slot):
        from mlcomp_amd.ops import _lib
        img, lab, par = slot
        dimg, dpar = self._dev[k % 2]
        cur = torch.cuda.current_stream(self.device)
        cs = self._copy_stream
        if self._used[k % 2] is not None:
            cs.wait_event(self._used[k % 2])
        with torch.cuda.stream(cs):
            dimg.copy_(img, non_blocking=True)
            dpar.copy_(par, non_blocking=True)
            dlab = lab.to(self.device, non_blocking=True)
            done = torch.cuda.Event()
            done.record(cs)
        cur.wait_event(done)
        dlab.record_stream(cur)
        shape, dt = self._out_shape(self.batch_size)
        out = torch.empty(shape, dtype=dt, device=self.device)
        _lib.call('mlc_augment', _lib.ptr(dimg), _lib.ptr(dpar), _lib.ptr(self._ms_dev), _lib.ptr(out),
                  self.batch_size, self.H, self.W, self.C, self.out_h, self.out_w, LAYOUTS[self.layout],
                  _lib.stream())
        used = torch.cuda.Event()
        used.record(cur)
        self._used[k % 2] = used
        return out, dlab, done

    def real_rows(self, k: int) -> int:
        """Samples of batch ``k`` that are not wrap-around padding.  Only the last batch of
        a ``drop_last=False`` epoch has padding: ``per - (len-1)*batch`` rows are real (the
        world-size padding of the shard stays, as DistributedSampler does it)."""
        if k < self._len - 1 or self._drop_last:
            return self.batch_size
        return self._per - (self._len - 1) * self.batch_size

    def __iter__(self):
        # an earlier iterator still alive holds an INUSE slot whose async H2D copy may be
        # pending: close it (its finally releases the slot) before the ring is reset
        prev = self._live() if self._live is not None else None
        if prev is not None:
            prev.close()
        gen = self._epoch_iter()
        self._live = weakref.ref(gen)
        return gen

    def _epoch_iter(self):
        rt = self._rt
        n = rt.mlr_loader_start_epoch(self._loader, self.epoch)
        if n < 0:
            raise RuntimeError('record loader: slots not registered')
        pending = None   # (slot index, copy-done event) of the previous batch
        bi = C.c_int64(0)
        try:
            for k in range(n):
                s = rt.mlr_loader_next(self._loader, C.byref(bi))
                if s < 0:
                    break
                slot = self._slots[s]
                if self.device.type == 'cuda':
                    x, y, done = self._augment_gpu(k, slot)
                else:
                    x, y = self._augment_cpu(slot)
                    done = None
                    rt.mlr_loader_release(self._loader, s)
                    s = -1
                if pending is not None:   # the previous slot's copy is long done: hand it back
                    ps, pev = pending
                    pev.synchronize()
                    rt.mlr_loader_release(self._loader, ps)
                pending = (s, done) if s >= 0 else None
                real = self.real_rows(k)
                if real < self.batch_size:   # drop the wrap-around rows of the last batch
                    x, y = x[:real], y[:real]
                yield {'features': x, 'targets': y}
        finally:
            if pending is not None:
                pending[1].synchronize()
                rt.mlr_loader_release(self._loader, pending[0])
            if not self._explicit_epoch:
                self.epoch += 1
            self._explicit_epoch = False

    def close(self):
        prev = self._live() if getattr(self, '_live', None) is not None else None
        if prev is not None:    # a live iterator hands its slot back before the loader goes
            prev.close()
        if getattr(self, '_loader', None):
            self._rt.mlr_loader_destroy(self._loader)
            self._loader = None
        if getattr(self, '_file', None):
            self._rt.mlr_close(self._file)
            self._file = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SegRecordLoader(RecordLoader):
    """Batches of an image + mask record file, on the ring, copy stream and events of
    :class:`RecordLoader`.

    ``train``: RandomResizedCrop(scale, ratio) + independent hflip / vflip / transpose coins,
    one transform for the image (bilinear) and its mask (nearest); otherwise the centre crop.
    ``out_size`` is an int or ``(h, w)``.  ``features`` come in ``layout``.  ``targets``:
    ``planes`` files give float 0/1 masks, ``[B, K, h, w]`` for ``mask_order='nkhw'`` (what
    torch criteria and the native eval path take) or pixel order ``[B, h, w, K]`` for
    ``'pixel'`` (what ``NativeSegmentationStep.load_batch(..., pixel_order=True)`` copies
    straight into its static buffer); ``index`` files give int64 class ids ``[B, h, w]``."""

    PAR = 8

    def __init__(self, path: str, batch_size: int, out_size=256, train: bool = True, scale=(0.5, 1.0),
                 ratio=(3 / 4, 4 / 3), layout: str = 'nchw', mask_order: str = 'nkhw', **kw):
        if mask_order not in ('nkhw', 'pixel'):
            raise ValueError(f'mask_order: nkhw / pixel, not {mask_order!r}')
        self.mask_order = mask_order
        super().__init__(path, batch_size, out_size=out_size, train=train, scale=scale, ratio=ratio,
                         layout=layout, **kw)

    def _open(self, path):
        rt = self._rt
        self._file = rt.mlr_seg_open(path.encode())
        if not self._file:
            raise ValueError(f'{path}: cannot open image + mask record file')
        shp = (C.c_uint64 * 6)()
        rt.mlr_seg_shape(self._file, shp)
        self.count, self.H, self.W, self.C, self.K, kind = (int(v) for v in shp)
        self.mask_kind = 'index' if kind else 'planes'
        self._create, self._set_slot = rt.mlr_seg_loader_create, rt.mlr_seg_loader_set_slot

    def _target_buffer(self, **kw):
        return torch.empty(self.batch_size, self.H, self.W, self.K, dtype=torch.uint8, **kw)

    def _staging(self):
        img, par = super()._staging()
        return img, self._target_buffer(device=self.device), par

    def _order(self, m):
        if self.mask_kind == 'planes' and self.mask_order == 'nkhw':
            return m.permute(0, 3, 1, 2).contiguous()
        return m

    def _augment_cpu(self, slot):
        img, mask, par = slot
        x, m = augment_seg_reference(img, mask, par, self.out_h, self.out_w, self.mean_istd, self.layout,
                                     self.mask_kind)
        return x, self._order(m)

    def _augment_gpu(self, k, slot):
        from mlcomp_amd.ops import _lib
        img, mask, par = slot
        dimg, dmask, dpar = self._dev[k % 2]
        cur = torch.cuda.current_stream(self.device)
        cs = self._copy_stream
        if self._used[k % 2] is not None:
            cs.wait_event(self._used[k % 2])
        with torch.cuda.stream(cs):
            dimg.copy_(img, non_blocking=True)
            dmask.copy_(mask, non_blocking=True)
            dpar.copy_(par, non_blocking=True)
            done = torch.cuda.Event()
            done.record(cs)
        cur.wait_event(done)
        B = self.batch_size
        shape, dt = self._out_shape(B)
        out = torch.empty(shape, dtype=dt, device=self.device)
        if self.mask_kind == 'index':
            m = torch.empty(B, self.out_h, self.out_w, dtype=torch.int64, device=self.device)
        else:
            m = torch.empty(B, self.out_h, self.out_w, self.K, dtype=torch.float32, device=self.device)
        _lib.call('mlc_augment_seg', _lib.ptr(dimg), _lib.ptr(dmask), _lib.ptr(dpar), _lib.ptr(self._ms_dev),
                  _lib.ptr(out), _lib.ptr(m), B, self.H, self.W, self.C, self.K, self.out_h, self.out_w,
                  LAYOUTS[self.layout], MASK_KINDS[self.mask_kind], _lib.stream())
        used = torch.cuda.Event()
        used.record(cur)
        self._used[k % 2] = used
        return out, self._order(m), done


class ClipRecordLoader(RecordLoader):
    """Batches of a clip record file, on the ring, copy stream and events of
    :class:`RecordLoader`: ``features`` logical ``[B, C, clip_len, h, w]``, ``targets`` int64
    ``[B]``.

    A clip is ``clip_len`` frames ``frame_stride`` apart; its span ``(clip_len-1) *
    frame_stride + 1`` must fit into the file's frames per record.  ``train``: one
    RandomResizedCrop(scale, ratio) box and one horizontal flip for the whole clip (the draws
    of :class:`RecordLoader`) and a random first frame; otherwise the centre crop of the
    centre frames, in file order.  Only the selected frames are copied into the ring and to
    the device.  ``out_size`` is an int or ``(h, w)``.  ``layout``: ``'ncthw'`` fp32
    contiguous (the torch engine), ``'nthwc'`` bf16 in channels_last_3d storage (a permuted
    view of ``[B, T, h, w, C]``, what the generic native engine's 3D sites read)."""

    PAR = 8
    LAYOUT_NAMES = CLIP_LAYOUTS

    def __init__(self, path: str, batch_size: int, clip_len: int, frame_stride: int = 1, out_size=112,
                 train: bool = True, scale=(0.3, 1.0), ratio=(3 / 4, 4 / 3), layout: str = 'ncthw', **kw):
        self.clip_len, self.frame_stride = int(clip_len), int(frame_stride)
        super().__init__(path, batch_size, out_size=out_size, train=train, scale=scale, ratio=ratio,
                         layout=layout, **kw)

    def _open(self, path):
        rt = self._rt
        self._file = rt.mlr_clip_open(path.encode())
        if not self._file:
            raise ValueError(f'{path}: cannot open clip record file')
        shp = (C.c_uint64 * 5)()
        rt.mlr_clip_shape(self._file, shp)
        self.count, self.H, self.W, self.C, self.F = (int(v) for v in shp)
        T, s = self.clip_len, self.frame_stride
        if T < 1 or s < 1 or (T - 1) * s + 1 > self.F:
            raise ValueError(f'{path}: clip_len T={T} at frame_stride s={s} spans {(T - 1) * s + 1} frames, '
                             f'the records hold F={self.F}')
        self._create = lambda f, batch, oh, ow, *rest: rt.mlr_clip_loader_create(f, batch, oh, ow, T, s, *rest)
        self._set_slot = rt.mlr_clip_loader_set_slot

    def _image_buffer(self, **kw):
        return torch.empty(self.batch_size, self.clip_len, self.H, self.W, self.C, dtype=torch.uint8, **kw)

    def _out_shape(self, B):
        if self.layout == 'nthwc':
            return (B, self.clip_len, self.out_h, self.out_w, self.C), torch.bfloat16
        return (B, self.C, self.clip_len, self.out_h, self.out_w), torch.float32

    def _augment_cpu(self, slot):
        img, lab, par = slot
        return augment_clip_reference(img, par, self.out_h, self.out_w, self.mean_istd, self.layout), lab.clone()

    def _augment_gpu(self, k, slot):
        from mlcomp_amd.ops import _lib
        img, lab, par = slot
        dimg, dpar = self._dev[k % 2]
        cur = torch.cuda.current_stream(self.device)
        cs = self._copy_stream
        if self._used[k % 2] is not None:
            cs.wait_event(self._used[k % 2])
        with torch.cuda.stream(cs):
            dimg.copy_(img, non_blocking=True)
            dpar.copy_(par, non_blocking=True)
            dlab = lab.to(self.device, non_blocking=True)
            done = torch.cuda.Event()
            done.record(cs)
        cur.wait_event(done)
        dlab.record_stream(cur)
        shape, dt = self._out_shape(self.batch_size)
        out = torch.empty(shape, dtype=dt, device=self.device)
        _lib.call('mlc_augment_clip', _lib.ptr(dimg), _lib.ptr(dpar), _lib.ptr(self._ms_dev), _lib.ptr(out),
                  self.batch_size, self.clip_len, self.H, self.W, self.C, self.out_h, self.out_w,
                  CLIP_LAYOUTS[self.layout], _lib.stream())
        used = torch.cuda.Event()
        used.record(cur)
        self._used[k % 2] = used
        if self.layout == 'nthwc':
            out = out.permute(0, 4, 1, 2, 3)
        return out, dlab, done


# ------------------------------------------------------------------------- text
def text_slot_ints(max_tokens: int, max_seqs: int) -> Tuple[int, int]:
    """(ints that cross to the device, ints of the whole slot) of a text loader slot:
    ``{nseq, total}``, ``{length, type0_length, label}[max_seqs]``, ``tokens[max_tokens]``, then
    - 8-byte aligned, host only - ``int64 indices[max_seqs]``."""
    head = 2 + 3 * max_seqs + max_tokens
    return head, ((head + 1) & ~1) + 2 * max_seqs


def text_unpack_reference(slot: torch.Tensor, T: int, nmax: int, max_len: int, vocab: int, num_labels: int,
                          layout: str = 'packed'):
    """PyTorch twin of ``mlc_text_unpack``: the int32 ``slot`` a text loader staged ->
    ``(tensors, err)``.  ``packed``: ``ids`` / ``tt`` / ``pos_ids`` int64 [T], ``cu`` int32
    [nmax + 1], ``y`` int64 [nmax], ``slot_w`` f32 [nmax]; ``padded``: ``input_ids`` /
    ``token_type_ids`` / ``attention_mask`` int64 [nmax, max_len] and ``y``.  The clamps are
    the kernel's (``csrc/kernels/text.hip``) and ``err`` counts them as its counter does."""
    if layout not in TEXT_LAYOUTS:
        raise ValueError(f'text layout: {" / ".join(TEXT_LAYOUTS)}, not {layout!r}')
    s = slot.detach().cpu().to(torch.int64)
    nseq = min(max(int(s[0]), 0), nmax)
    err = int(nseq != int(s[0]))
    ent = s[2:2 + 3 * nmax].view(nmax, 3)[:nseq]
    tok = s[2 + 3 * nmax:2 + 3 * nmax + T]
    cu = torch.zeros(nseq + 1, dtype=torch.int64)
    cu[1:] = torch.cumsum(ent[:, 0].clamp(0, max_len), 0).clamp(max=T)
    lens = cu[1:] - cu[:-1]
    total = int(cu[-1])
    err += int((lens != ent[:, 0]).sum()) + int(int(s[1]) != total)
    t0 = torch.minimum(ent[:, 1].clamp(min=0), lens)
    lab = ent[:, 2].clamp(0, num_labels - 1)
    err += int((t0 != ent[:, 1]).sum()) + int((lab != ent[:, 2]).sum())
    seq = torch.repeat_interleave(torch.arange(nseq), lens)
    q = torch.arange(total) - cu[:-1][seq]
    ids = tok[:total].clamp(0, vocab - 1)
    err += int((ids != tok[:total]).sum())
    tt = (q >= t0[seq]).long()
    y = torch.zeros(nmax, dtype=torch.long)
    y[:nseq] = lab
    if layout == 'padded':
        out = {k: torch.zeros(nmax, max_len, dtype=torch.long)
               for k in ('input_ids', 'token_type_ids', 'attention_mask')}
        out['input_ids'][seq, q] = ids
        out['token_type_ids'][seq, q] = tt
        out['attention_mask'][seq, q] = 1
        out['y'] = y
        return out, err
    out = {k: torch.zeros(T, dtype=torch.long) for k in ('ids', 'tt', 'pos_ids')}
    out['ids'][:total] = ids
    out['tt'][:total] = tt
    out['pos_ids'][:total] = q
    out['cu'] = torch.full((nmax + 1,), total, dtype=torch.int32)
    out['cu'][:nseq + 1] = cu.to(torch.int32)
    out['y'] = y
    nreal = int((lens > 0).sum())
    out['slot_w'] = torch.zeros(nmax, dtype=torch.float32)
    if nreal:
        out['slot_w'][:nseq] = (lens > 0).float() / nreal
    return out, err


class PackedTextBatch:
    """One batch a :class:`TextRecordLoader` staged, not yet unpacked: ``nseq`` sequences of
    ``tokens`` tokens in all (host ints), built for a step of ``T`` token rows, ``nmax``
    slots and sequences up to ``max_len``.  :meth:`unpack_into` writes the six tensors a
    packed ``NativeBertStep`` reads into the caller's buffers, with one kernel launch on the
    current stream; :meth:`tensors` allocates them."""

    def __init__(self, loader, staged, done, nseq, tokens):
        self._loader, self._staged, self._done = loader, staged, done
        self.nseq, self.tokens = int(nseq), int(tokens)
        self.T, self.nmax, self.max_len = loader.T, loader.max_seqs, loader.max_len
        self.vocab, self.num_labels = loader.vocab_size, loader.num_labels

    def unpack_into(self, ids, tt, pos_ids, cu, y, slot_w):
        outs = (ids, tt, pos_ids, cu, y, slot_w)
        want = ((self.T, torch.int64),) * 3 + ((self.nmax + 1, torch.int32), (self.nmax, torch.int64),
                                               (self.nmax, torch.float32))
        for t, (n, dt) in zip(outs, want):
            if t.numel() != n or t.dtype != dt or not t.is_contiguous() or t.device != self._staged.device:
                raise ValueError(f'unpack_into: a contiguous {dt} buffer of {n} elements on '
                                 f'{self._staged.device} expected, got {tuple(t.shape)} {t.dtype} on {t.device}')
        self._loader._unpack(self._staged, self._done, 'packed', outs)

    def tensors(self):
        dev = self._staged.device
        z = lambda n, dt: torch.empty(n, dtype=dt, device=dev)  # noqa: E731
        out = {'ids': z(self.T, torch.int64), 'tt': z(self.T, torch.int64), 'pos_ids': z(self.T, torch.int64),
               'cu': z(self.nmax + 1, torch.int32), 'y': z(self.nmax, torch.int64),
               'slot_w': z(self.nmax, torch.float32)}
        self.unpack_into(*out.values())
        return out


class TextRecordLoader(RecordLoader):
    """Batches of a text record file, on the slot ring and copy stream of :class:`RecordLoader`.

    A batch holds whole sequences: at most ``batch_size`` of them and ``pack_tokens`` tokens
    (default ``batch_size * max_len``: plain batches of ``batch_size``), filled greedily in
    the epoch's order by the rule of ``TokenBudgetBatchSampler``; the C++ runtime plans the
    epoch.  ``train`` shuffles per epoch and, with ``world_size > 1``, runs every rank for
    the step count of the rank with the fewest; otherwise file order and all of the rank's
    batches.  The file's longest record must fit ``max_len`` (truncate when packing).

    ``layout='padded'`` yields ``{'input_ids', 'token_type_ids', 'attention_mask',
    'targets'}`` on ``device``, ``[n, max_len]`` for the batch's n sequences, and
    ``'indices'`` (the record numbers, on the host).  ``layout='packed'`` yields ``{'packed':
    PackedTextBatch, 'targets', 'indices'}`` (both on the host) for
    ``NativeBertStep.load_text_batch``.  ``vocab_size`` is the model's: a file with a larger
    vocabulary is refused.  Token ids or labels out of range never reach the model: the
    unpack kernel clamps them and counts; :meth:`bad_tokens` reads the count, and the iterator
    raises ``ValueError`` at the end of an epoch that had any.  ``drop_last`` (plain batches
    only) skips a last batch of fewer than ``batch_size`` sequences, for engines of a fixed
    batch shape."""

    def __init__(self, path: str, batch_size: int, max_len: int = 128, pack_tokens: Optional[int] = None,
                 train: bool = True, layout: str = 'packed', vocab_size: Optional[int] = None, num_labels: int = 2,
                 seed: int = 0, rank: int = 0, world_size: int = 1, shuffle: Optional[bool] = None,
                 threads: int = 4, depth: int = 4, device=None, chunk: int = 16, drop_last: bool = False):
        if layout not in TEXT_LAYOUTS:
            raise ValueError(f'text layout: {" / ".join(TEXT_LAYOUTS)}, not {layout!r}')
        if drop_last and pack_tokens is not None:
            raise ValueError('drop_last is for plain batches (pack_tokens=None): a token-budget batch has no full size')
        self.drop_last = bool(drop_last)
        self.path, self.layout, self.train = path, layout, bool(train)
        self.batch_size = self.max_seqs = int(batch_size)
        self.max_len = int(max_len)
        self.max_tokens = int(pack_tokens) if pack_tokens is not None else self.max_seqs * self.max_len
        self.T = (self.max_tokens + 7) // 8 * 8          # token rows of the device tensors
        self.num_labels = int(num_labels)
        self.device = torch.device(device or ('cuda' if torch.cuda.is_available() else 'cpu'))
        self.epoch = 0
        self._explicit_epoch = False
        self._live = None
        self._planned = None                              # (epoch, steps) the runtime has started
        rt = self._rt = runtime()
        self._file = rt.mlr_text_open(path.encode())
        if not self._file:
            raise ValueError(f'{path}: cannot open text record file')
        shp = (C.c_uint64 * 5)()
        rt.mlr_text_shape(self._file, shp)
        self.count, self.file_max_len, self.file_vocab, self.token_bytes, self.total_tokens = (int(v) for v in shp)
        if vocab_size is not None and self.file_vocab > int(vocab_size):
            raise ValueError(f'{path}: the file was packed with a vocabulary of {self.file_vocab} tokens, the '
                             f'model has vocab_size = {int(vocab_size)}')
        self.vocab_size = int(vocab_size) if vocab_size is not None else self.file_vocab
        if not 1 <= self.max_seqs <= 1024:
            raise ValueError(f'batch_size {self.max_seqs}: 1 .. 1024 sequences per batch')
        if self.file_max_len > self.max_len:
            raise ValueError(f'{path}: the longest record has {self.file_max_len} tokens, over max_len = '
                             f'{self.max_len} (pack with --max-len {self.max_len})')
        if self.max_len > self.max_tokens or (layout == 'packed' and self.max_tokens % 8):
            raise ValueError(f'pack_tokens {self.max_tokens}: at least max_len = {self.max_len}'
                             + (', a multiple of 8' if layout == 'packed' else ''))
        shuffle = self.train if shuffle is None else shuffle
        self._rank, self._world = int(rank), int(world_size)
        self._loader = rt.mlr_text_loader_create(self._file, self.max_tokens, self.max_seqs, self.max_len,
                                                 int(self.train), int(seed), int(rank), int(world_size),
                                                 int(shuffle), int(threads), int(chunk))
        if not self._loader:
            raise ValueError('bad loader arguments')
        cuda = self.device.type == 'cuda'
        self._head, ints = text_slot_ints(self.max_tokens, self.max_seqs)
        self._slots = []
        for i in range(max(3, int(depth))):
            buf = torch.zeros(ints, dtype=torch.int32, pin_memory=cuda)
            rt.mlr_text_loader_set_slot(self._loader, i, C.c_void_p(buf.data_ptr()))
            self._slots.append(buf)
        self._err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._err_cpu = 0
        if cuda:
            self._copy_stream = torch.cuda.Stream(self.device)

    def _start(self):
        """Plan and start ``self.epoch`` in the runtime (once: ``len()`` before the epoch's
        iterator starts it early, and the workers prefetch from then on)."""
        if self._planned is None or self._planned[0] != self.epoch:
            n = self._rt.mlr_loader_start_epoch(self._loader, self.epoch)
            if n < 0:
                raise RuntimeError('record loader: slots not registered')
            self._planned = (self.epoch, int(n))
        return self._planned[1]

    def _short_last(self, steps):
        """Whether the last of ``steps`` plain batches is short and ``drop_last`` drops it: the
        rank holds every world-th record, ``batch_size`` to a batch."""
        own = len(range(self._rank, self.count, self._world))
        return self.drop_last and steps > 0 and steps * self.max_seqs > own

    def __len__(self):
        live = self._live() if self._live is not None else None
        if live is not None and self._planned is not None and live.gi_frame is not None:
            n = self._planned[1]                          # mid-epoch: the running epoch's plan
        else:
            n = self._start()
        return n - int(self._short_last(n))

    def bad_tokens(self) -> int:
        """Clamps the unpack kernel had to apply since the last check (a sync point)."""
        return int(self._err.item()) if self.device.type == 'cuda' else self._err_cpu

    def _unpack(self, staged, done, layout, outs):
        nmax, T = self.max_seqs, self.T
        if self.device.type != 'cuda':
            ref, err = text_unpack_reference(staged, T, nmax, self.max_len, self.vocab_size, self.num_labels, layout)
            for dst, src in zip(outs, ref.values()):
                dst.view(src.shape).copy_(src)
            self._err_cpu += err
            return
        from mlcomp_amd.ops import _lib
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(done)
        staged.record_stream(cur)       # its memory goes back to the copy stream's pool after this launch
        if layout == 'packed':
            ids, tt, pos, cu, y, w = outs
        else:
            (ids, tt, pos, y), cu, w = outs, None, None
        _lib.call('mlc_text_unpack', _lib.ptr(staged), TEXT_LAYOUTS[layout], _lib.ptr(ids), _lib.ptr(tt),
                  _lib.ptr(pos), _lib.ptr(cu), _lib.ptr(y), _lib.ptr(w), _lib.ptr(self._err), T, nmax, self.max_len,
                  self.vocab_size, self.num_labels, _lib.stream())

    def _stage(self, buf):
        """The device copy of a slot's head (its own tensor per batch, so a later batch's copy
        never lands in memory an earlier batch's unpack has yet to read) and the copy's event."""
        if self.device.type != 'cuda':
            return buf[:self._head].clone(), None
        with torch.cuda.stream(self._copy_stream):
            staged = torch.empty(self._head, dtype=torch.int32, device=self.device)
            staged.copy_(buf[:self._head], non_blocking=True)
            done = torch.cuda.Event()
            done.record(self._copy_stream)
        return staged, done

    def _epoch_iter(self):
        rt = self._rt
        n = self._start()
        nmax, head = self.max_seqs, self._head
        ioff = (head + 1) & ~1
        pending = None   # (slot index, copy-done event) of the previous batch
        bi = C.c_int64(0)
        try:
            for k in range(n):
                s = rt.mlr_loader_next(self._loader, C.byref(bi))
                if s < 0:
                    break
                buf = self._slots[s]
                nseq, total = int(buf[0]), int(buf[1])
                if self.drop_last and nseq < nmax:
                    rt.mlr_loader_release(self._loader, s)
                    continue
                indices = buf[ioff:ioff + 2 * nmax].view(torch.int64)[:nseq].clone()
                targets = buf[2:2 + 3 * nmax].view(nmax, 3)[:nseq, 2].long()
                staged, done = self._stage(buf)
                if done is None:
                    rt.mlr_loader_release(self._loader, s)
                    s = -1
                if pending is not None:   # the previous slot's copy is long done: hand it back
                    pending[1].synchronize()
                    rt.mlr_loader_release(self._loader, pending[0])
                pending = (s, done) if s >= 0 else None
                if self.layout == 'packed':
                    yield {'packed': PackedTextBatch(self, staged, done, nseq, total), 'targets': targets,
                           'indices': indices}
                    continue
                z = lambda: torch.empty(nmax, self.max_len, dtype=torch.long, device=self.device)  # noqa: E731
                ids, tt, mask, y = z(), z(), z(), torch.empty(nmax, dtype=torch.long, device=self.device)
                self._unpack(staged, done, 'padded', (ids, tt, mask, y))
                yield {'input_ids': ids[:nseq], 'token_type_ids': tt[:nseq], 'attention_mask': mask[:nseq],
                       'targets': y[:nseq], 'indices': indices}
            bad = self.bad_tokens()
            if bad:
                self._err.zero_()
                self._err_cpu = 0
                raise ValueError(f'{self.path}: {bad} token ids / labels / lengths were out of range for '
                                 f'vocab_size = {self.vocab_size}, num_labels = {self.num_labels}, max_len = '
                                 f'{self.max_len} and were clamped')
        finally:
            if pending is not None:
                pending[1].synchronize()
                rt.mlr_loader_release(self._loader, pending[0])
            self._planned = None
            if not self._explicit_epoch:
                self.epoch += 1
            self._explicit_epoch = False


__all__ = ['write_records', 'pack_images', 'RecordFile', 'RecordLoader', 'augment_reference', 'runtime',
           'write_seg_records', 'pack_seg_images', 'SegRecordFile', 'SegRecordLoader', 'augment_seg_reference',
           'write_clip_records', 'pack_clip_frames', 'ClipRecordFile', 'ClipRecordLoader', 'augment_clip_reference',
           'CLIP_LAYOUTS', 'TEXT_MAGIC', 'SEG_MAGIC', 'CLIP_MAGIC', 'write_text_records', 'pack_text_csv',
           'TextRecordFile', 'TextRecordLoader', 'PackedTextBatch', 'text_unpack_reference', 'text_slot_ints',
           'TEXT_LAYOUTS']
