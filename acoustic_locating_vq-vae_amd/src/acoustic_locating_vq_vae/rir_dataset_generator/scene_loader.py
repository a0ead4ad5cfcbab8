"""``SceneLoader`` -- training batches synthesised on the device, a room per sample, instead of read from a written dataset.

Where ``DeviceLoader`` serves what ``write_specs_dataset`` wrote (one room, one T60, one receiver for the whole set), this
loader keeps a pool of clean utterances in device memory and makes every batch from scratch:

    loader = SceneLoader(waves, 64, SceneConfig(), seed=0)
    speech, rir, echoed, fs, theta, wiener = next(iter(loader))      # DeviceLoader's 6-tuple, (64, 201, 500) spectrograms
    loader.last_scenes                                                # rooms, receivers, sources, T60, beta, theta

Per batch: B utterances drawn with replacement and one random crop of (500 - 1) * HOP_LENGTH samples each (exactly 500
STFT frames), B scenes from ``sample_scenes``, then RIR (csrc/rir.hip, one launch for all rooms) -> FIR -> STFT -> Wiener.
Every draw comes from one device generator seeded with ``seed``, so the batches depend on the seed only, and a batch step
makes no host sync: a loop can keep several batches in flight.  The config's checks guarantee valid scenes, so the per-item
checks of ``scene_impulse_responses`` (which sync) are not made here.
"""
import numpy as np
import torch

from .. import front_end as FE
from ..data_preprocessing import SPEC_FRAMES


class SceneLoader:
    def __init__(self, waves, batch_size, scene_config=None, seed=0, device="cuda"):
        """waves: clean utterances, a list of 1-D tensors / arrays or a 2-D tensor (one per row), copied to ``device`` as
        float32.  Utterances shorter than (500 - 1) * HOP_LENGTH samples give fewer than 500 frames and are dropped (the
        collate's rule); ``dropped`` counts them."""
        self.config = scene_config if scene_config is not None else FE.SceneConfig()
        if not isinstance(self.config, FE.SceneConfig):
            raise ValueError("SceneLoader: scene_config must be a front_end.SceneConfig")
        self.batch_size = int(batch_size)
        if self.batch_size <= 0:
            raise ValueError("SceneLoader: batch_size must be > 0, got %r" % (batch_size,))
        self.device = torch.device(device)
        FE._check_device(torch.empty(0, device=self.device), "SceneLoader")
        self.crop = (SPEC_FRAMES - 1) * self.config.HOP_LENGTH
        rows = [torch.as_tensor(np.asarray(w) if not isinstance(w, torch.Tensor) else w).reshape(-1) for w in waves]
        kept = [w for w in rows if w.shape[0] >= self.crop]
        self.dropped = len(rows) - len(kept)
        if not kept:
            raise ValueError("SceneLoader: no utterance has the %d samples of %d frames" % (self.crop, SPEC_FRAMES))
        lengths = [w.shape[0] for w in kept]
        self._flat = torch.cat([w.to(torch.float32) for w in kept]).to(self.device)
        self._windows = self._flat.unfold(0, self.crop, 1)                    # (total - crop + 1, crop) view, no copy
        self._offsets = torch.tensor(np.cumsum([0] + lengths[:-1]), dtype=torch.float64, device=self.device)
        self._starts = torch.tensor([n - self.crop + 1 for n in lengths], dtype=torch.float64, device=self.device)
        self.num_utterances = len(kept)
        self._signal = self.config.signal_config()
        self._generator = torch.Generator(device=self.device).manual_seed(int(seed))
        self.last_scenes = None
        self.last_indices = None

    def __iter__(self):
        return self

    def __next__(self):
        B, g = self.batch_size, self._generator
        u = torch.rand((B, 2), dtype=torch.float64, device=self.device, generator=g)
        utt = (u[:, 0] * self.num_utterances).long().clamp_max(self.num_utterances - 1)
        n_starts = self._starts.index_select(0, utt)
        start = self._offsets.index_select(0, utt) + torch.minimum((u[:, 1] * n_starts).floor(), n_starts - 1.0)
        wave = self._windows.index_select(0, start.long())                  # (B, crop) float32, contiguous copy
        scenes = FE.sample_scenes(B, self.config, generator=g)
        speech, rir, echoed, fs, theta, wiener = FE._samples_from_scenes(wave, scenes, self._signal, self.config.c, check=False)
        self.last_scenes, self.last_indices = scenes, utt
        fs_t = torch.full((B,), fs, dtype=torch.int64, device=self.device)
        crop = lambda x: x[:, :, :SPEC_FRAMES].contiguous()                 # noqa: E731  (a no-op at this crop length)
        return crop(speech), crop(rir), crop(echoed), fs_t, theta.reshape(B, 1), wiener
