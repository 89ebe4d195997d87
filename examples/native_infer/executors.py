"""``type: valid_synthetic``: the valid equation executor over a seeded set of random images.
The score is the share of rows whose argmax equals the label drawn with the image; the
predictions are also written to ``out`` so that two engines can be compared row by row."""
import numpy as np
import torch

from mlcomp_amd.worker.executors import Executor
from mlcomp_amd.worker.executors.valid import Valid


class SyntheticImages(torch.utils.data.Dataset):
    def __init__(self, n=256, size=64, classes=10, seed=4, a=0, b=None):
        g = torch.Generator().manual_seed(seed)
        self.images = torch.randn(n, 3, size, size, generator=g)
        self.labels = torch.randint(0, classes, (n,), generator=g).numpy()
        self.a, self.b = a, n if b is None else b

    def __len__(self):
        return self.b - self.a

    def __getitem__(self, i):
        return {'features': self.images[self.a + i], 'targets': int(self.labels[self.a + i])}


@Executor.register
class ValidSynthetic(Valid):
    def __init__(self, out: str = None, rows: int = 256, **kwargs):
        super().__init__(part_size=128, **kwargs)
        self.out, self.rows = out, int(rows)
        self.preds, self.correct = [], []

    def create_base(self):
        self.data = SyntheticImages(self.rows)

    def count(self):
        return self.rows

    def adjust_part(self, part):
        self.x = SyntheticImages(self.rows, a=part[0], b=part[1])

    def score(self, preds):
        self.preds.append(np.asarray(preds))
        ok = (np.asarray(preds).argmax(1) == self.data.labels[self.part[0]:self.part[1]]).astype(np.float64)
        self.correct.extend(ok)
        return ok

    def score_final(self):
        if self.out:
            np.save(self.out, np.concatenate(self.preds))
        return float(np.mean(self.correct)) if self.correct else 0.0
