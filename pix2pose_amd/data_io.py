"""Training batches on the GPU: the reference's pix2pose_util/data_io.py: data_generator over runtime.train_patch_batch
(csrc/train_batch.hip).

The draws come from Python's `random` module in the reference's order (runtime.train_draws) and the shuffles from `np.random`, so
with both seeded alike, the same directory listings and colour=False a run yields the reference's batches (scikit-image 0.17 / 0.18).
The colour stage (seq_syn) follows imgaug's documented meaning with parameters from a numpy Generator seeded by `seed`; it is NOT
pinned to imgaug, whose random stream and float arithmetic are not reproduced.

    python -m pix2pose_amd.data_io <gpu> <train_xyz dir> <back dir> <n_batches> <out.npz>

dumps batches for inspection.
"""
from __future__ import annotations

import os
import random
from collections import OrderedDict

import numpy as np

from . import runtime


def read_background(path: str):
    """uint8 [H, W, 3] or [H, W]: a .npy array as it is, anything else through PIL."""
    if path.endswith(".npy"):
        a = np.load(path)
    else:
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError("%s: PIL is needed to read image files (uint8 .npy backgrounds need nothing)" % path) from e
        with Image.open(path) as im:
            if im.mode not in ("L", "RGB"):
                im = im.convert("RGB")
            a = np.asarray(im)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError("%s: a background must be uint8 [H, W, 3] or [H, W], not %s %s" % (path, a.dtype, a.shape))
    return np.ascontiguousarray(a)


class data_generator:
    """The reference's data_generator with get_patch_pair on the GPU.  data_dir: train_xyz/<obj> (the .npy patches of make_train_xyz);
    back_dir: background images (.npy uint8, or whatever PIL reads).  ctx: a runtime.Context (default: device 0's).  colour=False
    skips the colour stage; seed seeds its parameter generator only -- `random` and `np.random` stay the caller's, as in the reference."""

    CACHE = 64      # decoded backgrounds kept

    def __init__(self, data_dir, back_dir, batch_size=50, gan=True, imsize=128, res_x=640, res_y=480, ctx=None, colour=True, seed=None,
                 **kwargs):
        self.data_dir = data_dir
        self.back_dir = back_dir
        self.imsize = imsize
        self.batch_size = batch_size
        self.gan = gan
        self.backfiles = os.listdir(back_dir)
        self.datafiles = [f for f in os.listdir(data_dir) if f.endswith(".npy")]
        self.res_x = res_x
        self.res_y = res_y
        self.n_data = len(self.datafiles)
        self.n_background = len(self.backfiles)
        print("Total training views:", self.n_data)
        self.ctx = ctx if ctx is not None else runtime.default_context(0)
        self.colour = colour
        self._rng = np.random.default_rng(seed)
        self._n_samples = 0
        self._backs = OrderedDict()

    def _background(self, draw: float):
        fn = self.backfiles[int(draw * (self.n_background - 1))]
        if fn in self._backs:
            self._backs.move_to_end(fn)
            return self._backs[fn]
        img = read_background(os.path.join(self.back_dir, fn))
        self._backs[fn] = img
        if len(self._backs) > self.CACHE:
            self._backs.popitem(last=False)
        return img

    def _sample(self, v_id, batch_count):
        """The host part of one sample: the patch, the background its first draw names, and the draw record."""
        patch = np.load(os.path.join(self.data_dir, self.datafiles[v_id]))
        chosen = []

        def shape_of(draw):
            chosen.append(self._background(draw))
            return chosen[0].shape
        rec = runtime.train_draws(random, patch.shape, shape_of, batch_count)
        return patch, chosen[0], rec

    def _run(self, samples, device=False):
        colours = None
        if self.colour:
            colours = runtime.train_colours(self._rng, len(samples), self._n_samples)
        self._n_samples += len(samples)
        return runtime.train_patch_batch(self.ctx, [s[0] for s in samples], [s[1] for s in samples], [s[2] for s in samples], colours,
                                         self.imsize, device=device)

    def get_patch_pair(self, v_id, batch_count):
        """-> (src [S, S, 3], tgt [S, S, 3], mask [S, S]) float32 of one sample: the batched path with a batch of one."""
        src, tgt, mask = self._run([self._sample(v_id, batch_count)])
        return src[0], tgt[0], mask[0]

    def generator(self):
        """Yields (batch_src, batch_tgt, batch_tgt_disc, batch_prob), or (batch_src, batch_tgt) with gan=False, for ever: the
        reference's shuffle, wrap-around and batch_count cycle of 100, every batch assembled in one library call."""
        scene_seq = np.arange(self.n_data)
        np.random.shuffle(scene_seq)
        idx = 0
        batch_count = 0
        batch_tgt_disc = np.ones((self.batch_size,))
        samples = []
        while True:
            v_id = scene_seq[idx]
            idx += 1
            if idx >= scene_seq.shape[0]:
                idx = 0
                np.random.shuffle(scene_seq)
            samples.append(self._sample(v_id, batch_count))
            if len(samples) >= self.batch_size:
                src, tgt, mask = self._run(samples)
                samples = []
                batch_count += 1
                if batch_count >= 100:
                    batch_count = 0
                if self.gan:
                    yield src, tgt, batch_tgt_disc, mask[..., None]
                else:
                    yield src, tgt


def main(argv=None):
    import sys
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 5:
        print(__doc__)
        return 2
    gpu, data_dir, back_dir, n_batches, out = int(argv[0]), argv[1], argv[2], int(argv[3]), argv[4]
    gen = data_generator(data_dir, back_dir, ctx=runtime.Context(gpu))
    it = gen.generator()
    dump = {}
    for k in range(n_batches):
        src, tgt, disc, prob = next(it)
        dump.update({"src_%d" % k: src, "tgt_%d" % k: tgt, "disc_%d" % k: disc, "prob_%d" % k: prob})
    np.savez_compressed(out, **dump)
    print("wrote %d batches to %s" % (n_batches, out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
