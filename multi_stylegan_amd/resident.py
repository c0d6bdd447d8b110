"""The device-resident TLFM dataset: every file decoded once, the counts kept in HBM, one kernel launch per batch.

The reference re-reads the dataset every epoch: ``TFLMDatasetGAN.__getitem__`` (dataset/tlfm_dataset.py:128-198) decodes every
frame of every sample in the DataLoader workers of train_multi_stylegan.py:60-63 -- with ``overlap=True`` each frame
``sequence_length`` times -- and every batch is collated, staged, copied host-to-device and normalised.  A few hundred
trapped-cell sequences of 128 KiB frames fit in one MI355X's memory many times over, so here:

* ``ResidentTLFMStore`` holds every distinct frame once (``frames`` ``[N, H, W]`` uint16), each frame's integer minimum and
  maximum (``ranges`` ``[N, 2]``, computed once by ``msg_tlfm_frame_range``) and the frame ids of every dataset sample
  (``samples`` ``[S, C, T]``), built from a ``TFLMDatasetGAN``'s own sample list, from counts in memory, or from a saved store.
* ``gather_tlfm_batch`` builds a batch ``[B, C, T, H, W]`` from a table of frame ids: one ``msg_tlfm_gather`` launch
  (csrc/tlfm_prepare.hip) that gathers, normalises and flips -- the arithmetic of ``data.prepare_tlfm_batch``, bit for bit.
* ``ResidentTLFMFeed`` is the epoch loop: a shuffled, rank-sharded plan drawn on the host, uploaded once per epoch, then one
  launch per step on the compute stream.  No file I/O, worker process, pinned staging, copy or thread per step.
"""
import hashlib
from concurrent.futures import ThreadPoolExecutor
from typing import Iterator, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .data import _prepare_tlfm_host
from .elastic import ElasticDeformation
from .tlfm_dataset import read_tiff

FORMAT_VERSION = 1
MAX_READERS = 16


def _frame_ranges(frames: torch.Tensor) -> torch.Tensor:
    """``[N, 2]`` int32 (min, max) of every frame of a store: ``msg_tlfm_frame_range`` on the device, numpy on the host."""
    N, H, W = frames.shape
    if not frames.is_cuda:
        flat = frames.numpy().reshape(N, H * W)
        return torch.from_numpy(np.stack([flat.min(axis=1), flat.max(axis=1)], axis=1).astype(np.int32))
    dev = frames.device
    ranges = torch.empty((N, 2), dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        _lib.check(_lib.lib().msg_tlfm_frame_range(frames.data_ptr(), N, H, W, ranges.data_ptr(), _lib.stream_of(dev)),
                   "msg_tlfm_frame_range")
    return ranges


def _gather_device(frames, ranges, index, hflip, vertical_flip, gfp, rfp, out_dtype) -> torch.Tensor:
    """The launch itself: validated, contiguous device tensors in, a fresh batch out."""
    dev = frames.device
    B, C, T = index.shape
    N, H, W = frames.shape
    out = torch.empty((B, C, T, H, W), dtype=out_dtype, device=dev)
    with _lib.on_device(dev):
        with _lib.kernel_clock.span(("tlfm_gather", out_dtype), out.numel() * (2.0 + out.element_size())):
            _lib.check(_lib.lib().msg_tlfm_gather(frames.data_ptr(), ranges.data_ptr(), N, index.data_ptr(), _lib.ptr(hflip),
                                                  out.data_ptr(), _lib.dtype_code(out), B, C, T, H, W, int(bool(vertical_flip)),
                                                  float(gfp[0]), float(gfp[1]), float(rfp[0]), float(rfp[1]),
                                                  _lib.stream_of(dev)), "msg_tlfm_gather")
    return out


def gather_tlfm_batch(frames: torch.Tensor, ranges: torch.Tensor, index: torch.Tensor, hflip: Optional[torch.Tensor] = None, *,
                      vertical_flip: bool = True, gfp=(150., 2200.), rfp=(20., 2000.),
                      out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The batch ``out[b, c, t] = prepare(frames[index[b, c, t]])`` as ``out_dtype`` (float32 or bfloat16) ``[B, C, T, H, W]``:
    ``frames`` the store ``[N, H, W]`` (``torch.uint16``), ``ranges`` its ``[N, 2]`` int32 (min, max) per frame, ``index`` the
    ``[B, C <= 3, T]`` integer frame ids, ``hflip`` the per-sample mirror flags ``[B]`` or None; everything else as
    ``data.prepare_tlfm_batch``, whose result on the stacked frames this equals bit for bit in float32 (bright field
    normalised by its frame's own range, a constant frame NaN).

    Device tensors go through ``msg_tlfm_gather`` (one launch on the current stream, a fresh output tensor); a frame id outside
    ``[0, N)`` reads nothing and gives a frame of NaN.  CPU tensors go through a torch statement of the same arithmetic, and a
    CPU ``index`` with such an id raises ValueError."""
    if frames.ndim != 3 or frames.dtype != torch.uint16:
        raise ValueError(f"the store is [N, H, W] raw counts (torch.uint16), got {frames.dtype} {tuple(frames.shape)}")
    if ranges.shape != (frames.shape[0], 2) or ranges.dtype != torch.int32:
        raise ValueError(f"ranges is [N = {frames.shape[0]}, 2] torch.int32, got {ranges.dtype} {tuple(ranges.shape)}")
    if index.ndim != 3 or not 1 <= index.shape[1] <= 3:
        raise ValueError(f"expected [B, C <= 3, T] frame ids, got {tuple(index.shape)}")
    if index.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"frame ids are torch.int32 (or int64), got {index.dtype}")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"out_dtype {out_dtype}: float32 or bfloat16")
    if hflip is not None and hflip.numel() != index.shape[0]:
        raise ValueError(f"hflip holds {hflip.numel()} flags for {index.shape[0]} samples")
    devices = {t.device for t in (frames, ranges, index, hflip) if t is not None}
    if len(devices) != 1:
        raise ValueError(f"store, ranges, index and hflip live on one device, got {sorted(map(str, devices))}")
    N = frames.shape[0]
    if not frames.is_cuda:
        if index.numel() and (int(index.min()) < 0 or int(index.max()) >= N):
            raise ValueError(f"frame ids {int(index.min())} .. {int(index.max())} outside the store's [0, {N})")
        stack = torch.from_numpy(frames.numpy()[index.numpy()])                        # [B, C, T, H, W] counts
        return _prepare_tlfm_host(stack, hflip, vertical_flip, gfp, rfp, out_dtype)
    if not frames.is_contiguous():
        raise ValueError("the store must be contiguous (it is never copied per batch)")
    if index.numel() == 0 or frames.numel() == 0:
        return torch.empty((*index.shape, *frames.shape[1:]), dtype=out_dtype, device=frames.device)
    if hflip is not None:
        hflip = hflip.reshape(-1).to(torch.uint8).contiguous()
    return _gather_device(frames, ranges.contiguous(), index.to(torch.int32).contiguous(), hflip, vertical_flip, gfp, rfp,
                          out_dtype)


class ResidentTLFMStore:
    """The dataset in one place: ``frames`` ``[N, H, W]`` uint16 (every distinct file once), ``ranges`` ``[N, 2]`` int32 (each
    frame's minimum and maximum), ``samples`` ``[S, C, T]`` int32 (the frame ids of every sample, in the dataset's order; on the
    store's device) and ``paths`` (the N file names).  ``gfp`` / ``rfp`` / ``flip`` are the dataset's normalisation settings,
    the defaults of ``gather``.  ``len(store)`` is S."""

    def __init__(self, frames: torch.Tensor, samples: torch.Tensor, paths: Optional[Sequence[str]] = None, *,
                 gfp=(150., 2200.), rfp=(20., 2000.), flip: bool = True):
        if frames.ndim != 3 or frames.dtype != torch.uint16 or frames.numel() == 0:
            raise ValueError(f"the store is a non-empty [N, H, W] torch.uint16 tensor, got {frames.dtype} {tuple(frames.shape)}")
        samples = torch.as_tensor(samples)
        if samples.ndim != 3 or not 1 <= samples.shape[1] <= 3 or samples.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"samples is an integer [S, C <= 3, T] table of frame ids, got {samples.dtype} {tuple(samples.shape)}")
        table = samples.cpu().to(torch.int32).contiguous()
        if table.numel() and (int(table.min()) < 0 or int(table.max()) >= frames.shape[0]):
            raise ValueError(f"samples names frames {int(table.min())} .. {int(table.max())}, the store has {frames.shape[0]}")
        paths = [f"frame{n}" for n in range(frames.shape[0])] if paths is None else [str(p) for p in paths]
        if len(paths) != frames.shape[0]:
            raise ValueError(f"{len(paths)} paths for {frames.shape[0]} frames")
        self.frames = frames.contiguous()
        self.ranges = _frame_ranges(self.frames)
        self.samples_host = table                                     # the feed draws its per-epoch tables from this copy
        self.samples = table.to(frames.device)
        self.paths = paths
        self.gfp, self.rfp, self.flip = (float(gfp[0]), float(gfp[1])), (float(rfp[0]), float(rfp[1])), bool(flip)

    def __len__(self) -> int:
        return self.samples_host.shape[0]

    @property
    def device(self) -> torch.device:
        return self.frames.device

    @staticmethod
    def _check_room(nbytes: int, device: torch.device) -> None:
        free, total = torch.cuda.mem_get_info(device)
        if nbytes > free:
            raise RuntimeError(f"the resident store needs {nbytes / 2 ** 30:.2f} GiB on {device}, {free / 2 ** 30:.2f} GiB of "
                               f"{total / 2 ** 30:.2f} GiB are free: feed this dataset through TLFMDeviceFeed instead")

    @classmethod
    def from_frames(cls, frames, samples, paths: Optional[Sequence[str]] = None,
                    device: Optional[Union[str, torch.device]] = None, **settings) -> "ResidentTLFMStore":
        """A store from counts already in memory: ``frames`` a uint16 ``[N, H, W]`` tensor or array on the CPU or the device
        (moved to ``device`` when one is given), ``samples`` the ``[S, C, T]`` frame ids; ``settings``: gfp / rfp / flip."""
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if device is not None and torch.device(device) != frames.device:
            device = torch.device(device)
            if device.type == "cuda":
                cls._check_room(frames.numel() * 2 + frames.shape[0] * 8, device)
            frames = frames.to(device)
        return cls(frames, samples, paths, **settings)

    @classmethod
    def from_dataset(cls, dataset, device: Union[str, torch.device] = "cuda", workers: int = 8) -> "ResidentTLFMStore":
        """Every distinct file of ``dataset`` (a ``TFLMDatasetGAN``) read ONCE with ``read_tiff`` by at most ``workers`` (never
        more than 16) threads, uploaded to ``device``.  The samples are ``dataset.paths_to_dataset_samples`` themselves: trap and
        z-position rules, ``positions``, ``no_rfp`` / ``no_gfp``, ``overlap`` and ``sequence_length`` are whatever the dataset
        applied; frames shared by overlapping samples are stored once.  The dataset's gfp / rfp ranges and ``flip`` become the
        gather's defaults.  ValueError: frames of different sizes (naming the file), a dataset with a ``transformations``
        callable (the store holds counts; a callable works on float frames), an empty dataset."""
        if getattr(dataset, "transformations", None) is not None:
            raise ValueError("the dataset has a `transformations` callable, which works on float frames: the resident store "
                             "holds raw counts (use the feed's `elastic=` for the deformation)")
        kinds = 1 if dataset.no_gfp else (2 if dataset.no_rfp else 3)
        ids, table = {}, []
        for sample in dataset.paths_to_dataset_samples:
            table.append([[ids.setdefault(p, len(ids)) for p in paths] for paths in sample[:kinds]])
        if not table:
            raise ValueError("the dataset has no samples")
        paths = list(ids)                                             # (insertion order: id n is paths[n])
        device = torch.device(device)
        first = read_tiff(paths[0])
        N, (H, W) = len(paths), first.shape
        if device.type == "cuda":
            cls._check_room(N * H * W * 2 + N * 8, device)
        counts = np.empty((N, H, W), dtype=np.uint16)
        counts[0] = first

        def read(n):
            image = read_tiff(paths[n])
            if image.shape != (H, W):
                raise ValueError(f"{paths[n]}: a {image.shape[0]} x {image.shape[1]} frame in a dataset of {H} x {W} frames "
                                 f"({paths[0]})")
            counts[n] = image

        with ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_READERS, N))) as pool:
            for _ in pool.map(read, range(1, N)):
                pass
        return cls(torch.from_numpy(counts).to(device), torch.tensor(table, dtype=torch.int32), paths,
                   gfp=(dataset.gfp_min, dataset.gfp_max), rfp=(dataset.rfp_min, dataset.rfp_max), flip=dataset.flip)

    def save(self, path: str) -> None:
        """One uncompressed ``.npz``: the counts, ``samples``, ``paths``, the normalisation settings and the format version
        (``ranges`` is recomputed by ``load``: one launch)."""
        with open(path, "wb") as f:
            np.savez(f, version=np.int64(FORMAT_VERSION), frames=self.frames.cpu().numpy(), samples=self.samples_host.numpy(),
                     paths=np.array(self.paths, dtype=np.str_), settings=np.array([*self.gfp, *self.rfp], dtype=np.float64),
                     flip=np.bool_(self.flip))

    @classmethod
    def load(cls, path: str, device: Union[str, torch.device] = "cuda") -> "ResidentTLFMStore":
        """The store ``save`` wrote, on ``device``.  ValueError: another format version, missing or inconsistent arrays."""
        with np.load(path, allow_pickle=False) as z:
            missing = {"version", "frames", "samples", "paths", "settings", "flip"} - set(z.files)
            if missing:
                raise ValueError(f"{path}: not a resident store (no {sorted(missing)})")
            if int(z["version"]) != FORMAT_VERSION:
                raise ValueError(f"{path}: store format version {int(z['version'])}, this package reads version {FORMAT_VERSION}")
            frames, samples, paths, settings = z["frames"], z["samples"], z["paths"], z["settings"]
            flip = bool(z["flip"])
        if frames.ndim != 3 or frames.dtype != np.uint16 or samples.ndim != 3 or samples.dtype != np.int32 or \
                paths.shape != (frames.shape[0],) or settings.shape != (4,):
            raise ValueError(f"{path}: inconsistent store (frames {frames.dtype} {frames.shape}, samples {samples.dtype} "
                             f"{samples.shape}, {paths.shape} paths, {settings.shape} settings)")
        return cls.from_frames(frames, torch.from_numpy(samples), [str(p) for p in paths], device=device,
                               gfp=tuple(settings[:2]), rfp=tuple(settings[2:]), flip=flip)

    def gather(self, sample_ids, hflip: Optional[torch.Tensor] = None, **kw) -> torch.Tensor:
        """The ``[B, C, T, H, W]`` batch of the samples ``sample_ids`` (a sequence or an integer tensor ``[B]``); ``hflip``
        ``[B]`` flags on any device or None; ``kw``: ``gather_tlfm_batch``'s keyword arguments, by default the store's
        settings.  Ids on the host are bounds-checked (ValueError); ids in device memory are not read back -- one outside
        ``[0, S)`` gives a sample of NaN."""
        ids = torch.as_tensor(sample_ids).reshape(-1)
        if ids.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
            raise ValueError(f"sample ids are integers, got {ids.dtype}")
        ids = ids.long()
        S = len(self)
        if not ids.is_cuda:
            if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= S):
                raise ValueError(f"sample ids {int(ids.min())} .. {int(ids.max())} outside the store's [0, {S})")
            index = self.samples_host[ids].to(self.device)
        else:
            ok = (ids >= 0) & (ids < S)
            index = torch.where(ok[:, None, None], self.samples[ids.clamp(0, S - 1)], -1)
        if hflip is not None:
            hflip = torch.as_tensor(hflip).to(self.device)
        kw.setdefault("vertical_flip", self.flip)
        kw.setdefault("gfp", self.gfp)
        kw.setdefault("rfp", self.rfp)
        return gather_tlfm_batch(self.frames, self.ranges, index, hflip, **kw)


class ResidentTLFMFeed:
    """``for batch in ResidentTLFMFeed(store, batch_size)``: one epoch over a ``ResidentTLFMStore``, every batch one
    ``msg_tlfm_gather`` launch on the current stream.  Each iteration runs the next epoch (``set_epoch`` for resumed runs):
    its plan is drawn on the host, its frame-id table ``[steps, B, C, T]`` and flip flags ``[steps, B]`` are uploaded once, and
    every step reads a slice of those device tables -- no copy, thread or DataLoader per step.  Batches are fresh tensors and
    stay valid for as long as the consumer keeps them.  ``len(feed)`` is the steps per epoch of this rank.

    ``plan(epoch)``: a pure function of (seed, epoch, rank, world, len(store), batch_size, shuffle, drop_last), drawn from a
    private ``torch.Generator``.  All ranks share one permutation of the samples (``shuffle=False``: the dataset's order) and one
    uniform draw per sample (mirrored when it is ``< horizontal_flip_probability``); step k of the epoch is the next
    ``batch_size * world`` samples of the permutation, of which rank r takes the r-th ``batch_size``.  Every rank gets the same
    number of steps -- with ``drop_last`` the last ``len(store) % (batch_size * world)`` samples of the permutation sit the
    epoch out; without it the feed ends on a short batch, which only a single rank may do (ValueError otherwise: ranks with
    different batch counts deadlock their collectives).

    ``rank`` / ``world``: default to the process group's, or 0 / 1.  ``gather_kwargs``: ``gather_tlfm_batch``'s keyword
    arguments, by default the store's settings.

    ``elastic``: an ``elastic.ElasticDeformation``, exactly as in ``data.TLFMDeviceFeed``: every batch is deformed on the compute
    stream right after the gather (one field per sample, noise from the module's generator), in the dtype the gather wrote.
    The caveat stated there applies unchanged: the NORMALISED, FLIPPED frames are deformed, whereas the reference's ``Compose``
    deforms the counts BEFORE normalisation."""

    def __init__(self, store: ResidentTLFMStore, batch_size: int, *, shuffle: bool = True, drop_last: bool = True, seed: int = 0,
                 rank: Optional[int] = None, world: Optional[int] = None, horizontal_flip_probability: float = 0.5,
                 elastic: Optional[ElasticDeformation] = None, **gather_kwargs):
        if elastic is not None:
            if not isinstance(elastic, ElasticDeformation):
                raise ValueError(f"elastic is an ElasticDeformation or None, got {type(elastic).__name__}")
            if elastic.sample_mode != "bilinear":
                raise ValueError(f"sample_mode {elastic.sample_mode!r}: the device path samples bilinearly only")
        group = torch.distributed.is_available() and torch.distributed.is_initialized()
        self.rank = int(rank) if rank is not None else (torch.distributed.get_rank() if group else 0)
        self.world = int(world) if world is not None else (torch.distributed.get_world_size() if group else 1)
        self.store, self.batch_size = store, int(batch_size)
        if self.batch_size < 1 or self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError(f"batch_size {batch_size}, rank {self.rank} of {self.world}: a positive batch and 0 <= rank < world")
        if not drop_last and self.world > 1:
            raise ValueError(f"drop_last=False ends the epoch on a short batch, which {self.world} ranks cannot share: every rank "
                             "needs the same number of steps")
        self.shuffle, self.drop_last, self.seed = bool(shuffle), bool(drop_last), int(seed)
        self.horizontal_flip_probability = float(horizontal_flip_probability)
        self.elastic = elastic
        self.gather_kwargs = {"vertical_flip": store.flip, "gfp": store.gfp, "rfp": store.rfp, "out_dtype": torch.float32,
                              **gather_kwargs}
        unknown = set(self.gather_kwargs) - {"vertical_flip", "gfp", "rfp", "out_dtype"}
        if unknown:
            raise TypeError(f"unexpected keyword arguments {sorted(unknown)}")
        if self.gather_kwargs["out_dtype"] not in (torch.float32, torch.bfloat16):
            raise ValueError(f"out_dtype {self.gather_kwargs['out_dtype']}: float32 or bfloat16")
        per_step = self.batch_size * self.world
        self.steps = len(store) // per_step if self.drop_last else -(-len(store) // per_step)
        if self.steps == 0:
            raise ValueError(f"{len(store)} samples do not fill one step of {self.world} x {self.batch_size}")
        self.epoch = 0

    def __len__(self) -> int:
        return self.steps

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def plan(self, epoch: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(sample_ids [steps, B] int64, hflip [steps, B] uint8)`` of this rank in ``epoch``, on the CPU.  A short last batch
        (``drop_last=False``) is padded with id -1 / flag 0; the feed yields only the samples in front of the padding."""
        S, B = len(self.store), self.batch_size
        # (the CPU generator keeps 32 bits of a seed: (seed, epoch) is hashed into them, not packed side by side)
        digest = hashlib.sha256(f"msg-resident-feed:{self.seed}:{int(epoch)}".encode()).digest()
        g = torch.Generator().manual_seed(int.from_bytes(digest[:4], "little"))
        order = torch.randperm(S, generator=g) if self.shuffle else torch.arange(S)
        mirrored = (torch.rand(S, generator=g) < self.horizontal_flip_probability).to(torch.uint8)       # one draw per sample
        used = self.steps * B * self.world
        ids = torch.full((used,), -1, dtype=torch.int64)
        ids[:min(used, S)] = order[:used]
        ids = ids.view(self.steps, self.world, B)[:, self.rank].contiguous()
        flags = torch.where(ids >= 0, mirrored[ids.clamp(min=0)], torch.zeros((), dtype=torch.uint8))
        return ids, flags

    def __iter__(self) -> Iterator[torch.Tensor]:
        epoch, self.epoch = self.epoch, self.epoch + 1
        return self._run(epoch)

    def _run(self, epoch: int) -> Iterator[torch.Tensor]:
        store, kw = self.store, self.gather_kwargs
        ids, flags = self.plan(epoch)
        sizes = (ids >= 0).sum(dim=1).tolist()
        table = store.samples_host[ids.clamp(min=0)].to(store.device)            # [steps, B, C, T]: this epoch's only uploads
        flags = flags.to(store.device)
        on_host = not store.frames.is_cuda
        for k, size in enumerate(sizes):
            if on_host:
                batch = gather_tlfm_batch(store.frames, store.ranges, table[k, :size], flags[k, :size], **kw)
            else:
                batch = _gather_device(store.frames, store.ranges, table[k, :size], flags[k, :size], kw["vertical_flip"],
                                       kw["gfp"], kw["rfp"], kw["out_dtype"])
            yield batch if self.elastic is None else self.elastic.deform_batch(batch)
