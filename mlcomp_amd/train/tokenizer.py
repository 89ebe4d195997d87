"""WordPiece tokenisation for the text record packer (:func:`mlcomp_amd.train.records.pack_text_csv`).

BERT's two steps in plain Python: the basic tokeniser (whitespace clean-up, optional
lower-casing with accent stripping, punctuation split, every CJK character a token of its
own), then greedy longest-match-first WordPiece with ``##`` continuation pieces over a
``vocab.txt`` (one token per line, its line number the id).  It runs once, when a CSV is
packed; training reads the ids from the record file.
"""
from __future__ import annotations

import unicodedata
from typing import List, Optional, Tuple

MAX_WORD_CHARS = 100


def _is_whitespace(ch: str) -> bool:
    return ch in ' \t\n\r' or unicodedata.category(ch) == 'Zs'


def _is_control(ch: str) -> bool:
    return ch not in '\t\n\r' and unicodedata.category(ch).startswith('C')


def _is_punctuation(ch: str) -> bool:
    cp = ord(ch)
    # every non-letter, non-digit ASCII symbol counts ("$", "^", "`" are not Unicode class P)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True
    return unicodedata.category(ch).startswith('P')


def _is_cjk(cp: int) -> bool:
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F
            or 0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF
            or 0x2F800 <= cp <= 0x2FA1F)


class WordPieceTokenizer:
    """``vocab_path``: a BERT ``vocab.txt``; it must hold ``[CLS]``, ``[SEP]`` and ``[UNK]``.
    ``lower``: lower-case and strip accents (the uncased models)."""

    def __init__(self, vocab_path: str, lower: bool = True):
        self.vocab = {}
        with open(vocab_path, encoding='utf-8') as f:
            for line in f:
                tok = line.rstrip('\n')
                if tok and tok not in self.vocab:
                    self.vocab[tok] = len(self.vocab)
        missing = [t for t in ('[CLS]', '[SEP]', '[UNK]') if t not in self.vocab]
        if missing:
            raise ValueError(f'{vocab_path}: the vocabulary lacks {" ".join(missing)}')
        self.lower = bool(lower)
        self.cls_id, self.sep_id, self.unk_id = (self.vocab[t] for t in ('[CLS]', '[SEP]', '[UNK]'))

    # ------------------------------------------------------------------ basic tokeniser
    def basic(self, text: str) -> List[str]:
        """Words, punctuation marks and CJK characters of ``text``."""
        out = []
        for ch in text:
            cp = ord(ch)
            if cp == 0 or cp == 0xFFFD or _is_control(ch):
                continue
            if _is_whitespace(ch):
                out.append(' ')
            elif _is_cjk(cp):
                out.append(f' {ch} ')
            else:
                out.append(ch)
        words = []
        for word in ''.join(out).split():
            if self.lower:
                word = ''.join(c for c in unicodedata.normalize('NFD', word.lower())
                               if unicodedata.category(c) != 'Mn')
            cur = ''
            for ch in word:
                if _is_punctuation(ch):
                    if cur:
                        words.append(cur)
                    words.append(ch)
                    cur = ''
                else:
                    cur += ch
            if cur:
                words.append(cur)
        return words

    # ------------------------------------------------------------------ wordpiece
    def wordpiece(self, word: str) -> List[str]:
        """Greedy longest-match-first pieces of one word; ``[UNK]`` when some part of it has
        no piece, or the word is longer than 100 characters."""
        if len(word) > MAX_WORD_CHARS:
            return ['[UNK]']
        pieces, start = [], 0
        while start < len(word):
            end = len(word)
            piece = None
            while start < end:
                sub = ('##' if start else '') + word[start:end]
                if sub in self.vocab:
                    piece = sub
                    break
                end -= 1
            if piece is None:
                return ['[UNK]']
            pieces.append(piece)
            start = end
        return pieces

    def tokenize(self, text: str) -> List[str]:
        return [p for w in self.basic(text) for p in self.wordpiece(w)]

    def ids(self, text: str) -> List[int]:
        return [self.vocab[p] for p in self.tokenize(text)]

    def encode(self, text_a: str, text_b: Optional[str] = None, max_len: int = 128) -> Tuple[List[int], int]:
        """``([CLS] a [SEP]`` or ``[CLS] a [SEP] b [SEP]`` as ids, type0_length``)``: the first
        ``type0_length`` tokens (through the first ``[SEP]``) have token type 0, the rest 1.  The
        result has at most ``max_len`` tokens: a single text loses its tail, a pair is
        truncated longest-first (one token at a time off the end of the longer side, b on a
        tie)."""
        a = self.ids(text_a)
        if text_b is None:
            if max_len < 2:
                raise ValueError('max_len must leave room for [CLS] and [SEP]')
            a = a[:max_len - 2]
            return [self.cls_id] + a + [self.sep_id], len(a) + 2
        if max_len < 3:
            raise ValueError('max_len must leave room for [CLS] and two [SEP]')
        b = self.ids(text_b)
        while len(a) + len(b) > max_len - 3:
            (a if len(a) > len(b) else b).pop()
        return [self.cls_id] + a + [self.sep_id] + b + [self.sep_id], len(a) + 2


__all__ = ['WordPieceTokenizer']
