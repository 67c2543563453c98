"""Software pipeline behind ``Dataset.map`` for the encode jobs (VERDICT r2 "What's missing" 1).

The reference's ``embed`` (meerqat/ir/embedding.py:197-246, meerqat/image/embedding.py:125-166) is strictly serial per batch:
tokenise / decode on the CPU -> pageable synchronous ``.to(device)`` -> forward -> ``.cpu().numpy()`` -> Arrow write, so the
GPU idles during every host stage.  ``Dataset.map`` stays the driver here (same call, same batches, same output dataset), but
the function it calls is a :class:`Lookahead` step:

* a WORKER THREAD prepares batch j + 1 while the GPU runs batch j: it reads the batch's rows straight from the Arrow table,
  does the host work (tokenisation into PINNED buffers / image decoding and packing), issues the host -> device copies with
  ``non_blocking=True`` on a SIDE STREAM, builds whatever the forward would otherwise have to read back from the device (the
  packed-forward plan from the tokenizer's lengths) and records an event;
* the map function for batch i first LAUNCHES batch i + 1 on the compute stream (which waits for the worker's event on the
  device, not on the host), then waits for ONE event -- batch i's result landing in pinned memory -- and returns it.  The
  Arrow write of batch i (done by ``Dataset.map`` after the function returns) therefore overlaps the forward of batch i + 1.

Results are identical to the serial path: the same tokenizer backend (validated against ``tokenizer(texts, **kwargs)`` on the
first batch, else the tokenizer itself is called in the worker), the same forward.  Anything the prefetcher cannot know ahead
of ``Dataset.map`` (query expansion, KB features, shuffled / filtered datasets, ``num_proc``) keeps the serial path.
"""
import itertools
import os
import queue
import threading
import time
import types

import numpy as np
import torch


class _Failure:
    def __init__(self, exc):
        self.exc = exc


class Lookahead:
    """``prepare(j)`` (worker thread) -> prepared inputs of batch j; ``launch(prepared)`` (caller's thread) enqueues the
    device work and returns a handle whose ``result()`` blocks until batch j's output is on the host.  ``step(i)`` returns
    batch i's result after making sure batch i + 1 is already running."""

    def __init__(self, n_batches, prepare, launch, depth=2):
        self.n, self._prepare, self._launch = int(n_batches), prepare, launch
        self._q = queue.Queue(maxsize=max(1, int(depth)))
        self._handles = {}
        self._launched = 0
        self._stop = False
        self.wait_prepared_s = 0.0   # time the caller spent waiting for the worker (host-bound when this grows)
        self._thread = threading.Thread(target=self._work, name="viquae-amd-prefetch", daemon=True)
        self._thread.start()

    def _work(self):
        try:
            for j in range(self.n):
                if self._stop:
                    return
                item = self._prepare(j)
                while not self._stop:
                    try:
                        self._q.put(item, timeout=0.2)
                        break
                    except queue.Full:
                        continue
        except BaseException as e:  # noqa: BLE001 - handed to the caller's thread
            self._q.put(_Failure(e))

    def _launch_next(self):
        t0 = time.perf_counter()
        item = self._q.get()
        self.wait_prepared_s += time.perf_counter() - t0
        if isinstance(item, _Failure):
            self._stop = True
            raise item.exc
        self._handles[self._launched] = self._launch(item)
        self._launched += 1

    def step(self, i):
        if i < self._launched - len(self._handles) or i >= self.n:
            raise RuntimeError(f"batch {i} was requested out of order (batches must be taken in sequence)")
        while self._launched <= min(i + 1, self.n - 1):
            self._launch_next()
        return self._handles.pop(i).result()

    def close(self):
        self._stop = True
        try:
            while True:
                self._q.get_nowait()
        except queue.Empty:
            pass
        self._thread.join(timeout=5.0)
        self._handles.clear()


class _Handle:
    def __init__(self, event, pinned, rows, extra=None):
        self.event, self.pinned, self.rows, self.extra = event, pinned, rows, extra

    def result(self):
        if self.event is not None:
            self.event.synchronize()
        return np.array(self.pinned[: self.rows].numpy()), self.extra  # a copy: the pinned slot is reused two batches later


class _PinnedRing:
    """Page-locked staging slots, reused round-robin; a slot is handed out again only after the copy that read it is done."""

    def __init__(self, slots):
        self.bufs = [None] * slots
        self.events = [None] * slots
        self.next = 0

    def take(self, nbytes):
        s = self.next
        self.next = (s + 1) % len(self.bufs)
        if self.events[s] is not None:
            self.events[s].synchronize()
            self.events[s] = None
        if self.bufs[s] is None or self.bufs[s].numel() < nbytes:
            self.bufs[s] = torch.empty(int(nbytes * 5 // 4) + 64, dtype=torch.uint8, pin_memory=True)
        return s, self.bufs[s]


# ----------------------------------------------------------------------------------------------------------------------
# text
# ----------------------------------------------------------------------------------------------------------------------
class FastBatchTokenizer:
    """``tokenizer(texts, **tokenization_kwargs)`` for the plain case -- a list of single texts, ``return_tensors="pt"``,
    ``padding`` "max_length" / True / "longest", optional truncation -- computed from the tokenizer's own Rust backend
    (``tokenizer.backend_tokenizer``: same normaliser, pre-tokeniser, model and post-processor) without the per-element Python
    passes of ``BatchEncoding.convert_to_tensors`` (transformers 5: 0.86 s of a 0.95 s call for 2048 passages padded to 256).
    The backend releases the GIL and encodes in parallel; the padded int64 matrices are then built with numpy.  ``check()``
    compares with the tokenizer's own output and must pass before the fast path is trusted."""

    SUPPORTED = {"return_tensors", "padding", "truncation", "max_length"}

    def __init__(self, tokenizer, tokenization_kwargs):
        self.tokenizer, self.kwargs = tokenizer, dict(tokenization_kwargs)
        self.ok = False
        self.left = getattr(tokenizer, "padding_side", "right") == "left"
        backend = getattr(tokenizer, "backend_tokenizer", None) or getattr(tokenizer, "_tokenizer", None)
        kw = self.kwargs
        if backend is None or set(kw) - self.SUPPORTED or kw.get("return_tensors") != "pt":
            return
        padding = kw.get("padding", False)
        if padding not in ("max_length", True, "longest"):
            return
        truncation = kw.get("truncation", False)
        if truncation not in (True, False, "longest_first"):
            return
        max_length = kw.get("max_length")
        if max_length is None and (truncation or padding == "max_length"):
            mml = getattr(tokenizer, "model_max_length", None)
            max_length = int(mml) if mml is not None and mml < 1_000_000 else None
        if padding == "max_length" and max_length is None:
            return
        try:
            import tokenizers
            self.backend = tokenizers.Tokenizer.from_str(backend.to_str())  # a private copy: truncation / padding are state
        except Exception:
            return
        self.backend.no_padding()
        if truncation and max_length is not None:
            self.backend.enable_truncation(int(max_length))
        else:
            self.backend.no_truncation()
        self.pad_to = int(max_length) if padding == "max_length" else None
        self.pad_id = int(tokenizer.pad_token_id if tokenizer.pad_token_id is not None else 0)
        self.left = getattr(tokenizer, "padding_side", "right") == "left"
        self.names = list(getattr(tokenizer, "model_input_names", ["input_ids", "attention_mask"]))
        if not set(self.names) <= {"input_ids", "token_type_ids", "attention_mask"}:
            return
        self.ok = True

    def encode(self, texts):
        """-> (lengths int64 [B], flat ids int64 [sum lengths])"""
        enc = self.backend.encode_batch_fast(texts, add_special_tokens=True) if hasattr(self.backend, "encode_batch_fast") \
            else self.backend.encode_batch(texts, add_special_tokens=True)
        ids = [e.ids for e in enc]
        lens = np.fromiter(map(len, ids), dtype=np.int64, count=len(ids))
        flat = np.fromiter(itertools.chain.from_iterable(ids), dtype=np.int64, count=int(lens.sum()))
        return lens, flat

    def fill(self, lens, flat, out):
        """out: dict name -> int64 numpy [B, L] views to fill (the tokenizer's padded matrices)."""
        B, L = out["input_ids"].shape
        cols = np.arange(L, dtype=np.int64)[None, :]
        mask = (cols >= L - lens[:, None]) if self.left else (cols < lens[:, None])
        ids = out["input_ids"]
        ids.fill(self.pad_id)
        ids[mask] = flat
        if "attention_mask" in out:
            np.copyto(out["attention_mask"], mask, casting="unsafe")
        if "token_type_ids" in out:
            out["token_type_ids"].fill(0)  # single texts: every token belongs to segment 0 (pad_token_type_id is 0 too)

    def width(self, lens):
        return self.pad_to if self.pad_to is not None else int(lens.max()) if lens.size else 0

    def __call__(self, texts):
        lens, flat = self.encode(texts)
        L = self.width(lens)
        out = {n: np.empty((len(texts), L), dtype=np.int64) for n in self.names}
        self.fill(lens, flat, out)
        return {n: torch.from_numpy(a) for n, a in out.items()}, lens

    def check(self, texts):
        """True when the fast path reproduces ``tokenizer(texts, **kwargs)`` exactly (keys, order, dtypes, values)."""
        if not self.ok:
            return False
        try:
            want = self.tokenizer(texts, **self.kwargs)
            got, _ = self(texts)
            same = list(want.keys()) == list(got.keys()) and all(
                want[k].dtype == got[k].dtype and want[k].shape == got[k].shape and bool(torch.equal(want[k], got[k])) for k in got)
        except Exception:
            same = False
        self.ok = bool(same)
        return self.ok


def _arrow_strings(dataset, key):
    """The Arrow column ``key`` of a dataset without an indices mapping, or None."""
    import pyarrow as pa
    if getattr(dataset, "_indices", None) is not None or key not in dataset.column_names:
        return None
    col = dataset.data.column(key)
    if not (pa.types.is_string(col.type) or pa.types.is_large_string(col.type)):
        return None
    return col


def model_device(model):
    """The device of the model's first parameter, else of its first buffer (models that keep their weights as buffers only, like
    the ArcFace port); None for an object with neither."""
    first = next(iter(model.parameters()), None) if hasattr(model, "parameters") else None
    if first is None and hasattr(model, "buffers"):
        first = next(iter(model.buffers()), None)
    return None if first is None else first.device


class _EncodeJob:
    """The skeleton of the three encode jobs: batch bounds, device, streams, pinned output ring, :class:`Lookahead`, ``embed``.
    A job sets its own state, then calls ``_EncodeJob.__init__`` (the worker starts on batch 0 at once), and implements
    ``_prepare(j)`` (worker thread) -> dict(names = ``batch[key]``, event = side-stream event of the inputs or None when there
    is nothing to run, tensors = device tensors the forward reads, info = what ``_result`` needs, ...), ``_forward(p)`` -> the
    device result, one row per output row, and ``_result(batch, found, info)`` -> what ``Dataset.map`` gets back."""

    def __init__(self, dataset, model, key, batch_size, stats, depth=2):
        self.model, self.key = model, key
        n = len(dataset)
        self.bounds = [(s, min(s + batch_size, n)) for s in range(0, n, batch_size)]
        self.device = model_device(model)
        self.main = torch.cuda.current_stream(self.device)
        self.side = torch.cuda.Stream(device=self.device)
        self.out_ring = _PinnedRing(3)
        self.stats = {"batches": 0, "prepare_s": 0.0, "launch_s": 0.0, "wait_result_s": 0.0, **stats}
        self.look = Lookahead(len(self.bounds), self._prepare, self._launch, depth=depth)

    # ---- caller's thread -------------------------------------------------------------------------------------------
    def _launch(self, p):
        """Batch j's forward on the compute stream behind the worker's event, its float32 result copied to pinned memory."""
        t0 = time.perf_counter()
        extra = (p["names"], p["info"])
        if p["event"] is None:
            return _Handle(None, torch.empty((0, 1)), 0, extra=extra)
        with torch.cuda.device(self.device):
            self.main.wait_event(p["event"])
            for t in p["tensors"]:
                t.record_stream(self.main)
            with torch.no_grad():
                out = self._forward(p)
            out = out.to(torch.float32).contiguous()
            slot, buf = self.out_ring.take(out.numel() * 4)
            pinned = buf[: out.numel() * 4].view(torch.float32).view(out.shape)
            pinned.copy_(out, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.main)
            self.out_ring.events[slot] = ev
        self.stats["launch_s"] += time.perf_counter() - t0
        return _Handle(ev, pinned, out.shape[0], extra=extra)

    def embed(self, batch, indices):
        """The function ``Dataset.map`` calls (batched, with_indices) for THIS batch."""
        i = self.stats["batches"]
        s, e = self.bounds[i] if i < len(self.bounds) else (-1, -1)
        if len(indices) != e - s or int(indices[0]) != s or int(indices[-1]) != e - 1:
            raise RuntimeError("Dataset.map handed over batches in another order than the prefetcher prepared them "
                               f"(batch {i}: rows {indices[0]}..{indices[-1]}, expected {s}..{e - 1}); set MQ_EMBED_PIPELINE=0")
        t0 = time.perf_counter()
        found, (names, info) = self.look.step(i)
        self.stats["wait_result_s"] += time.perf_counter() - t0
        if names != batch[self.key]:
            raise RuntimeError(f"the prefetched '{self.key}' of batch {i} differ from what Dataset.map decoded; set MQ_EMBED_PIPELINE=0")
        self.stats["batches"] = i + 1
        self.stats.setdefault("returned_at", []).append(time.perf_counter())  # per batch: lets a caller separate start-up from pace
        return self._result(batch, found, info)

    def close(self):
        self.stats["wait_prepared_s"] = self.look.wait_prepared_s
        self.look.close()


# ----------------------------------------------------------------------------------------------------------------------
# text
# ----------------------------------------------------------------------------------------------------------------------
class TextEmbedPipeline(_EncodeJob):
    """``embed`` for ``Dataset.map(..., batched=True, with_indices=True)`` with the host stages of batch i + 1 (Arrow ->
    str, tokenisation, pinned staging, H2D, packed-forward plan) hidden behind the forward of batch i.  Plain passages /
    questions only (no query expansion, no KB features, no per-layer dump): see :func:`text_pipeline_or_none`."""

    def __init__(self, dataset, model, tokenizer, tokenization_kwargs, key, save_as, output_key, forward_kwargs, call, batch_size,
                 depth=2):
        self.save_as, self.output_key = save_as, output_key
        self.forward_kwargs, self.call = dict(forward_kwargs or {}), call
        self.tokenizer, self.tokenization_kwargs = tokenizer, dict(tokenization_kwargs or {})
        self.column = _arrow_strings(dataset, key)
        self.fast = FastBatchTokenizer(tokenizer, self.tokenization_kwargs)
        self._checked = False
        self.use_plan = bool(getattr(model, "supports_pack_plan", False)) and call is None and not self.fast.left
        self.in_ring = _PinnedRing(depth + 2)
        super().__init__(dataset, model, key, batch_size, {"tokenize_s": 0.0, "fast_tokenizer": None, "pack_plan": self.use_plan},
                         depth=depth)

    # ---- worker thread ---------------------------------------------------------------------------------------------
    def _prepare(self, j):
        t0 = time.perf_counter()
        s, e = self.bounds[j]
        texts = self.column.slice(s, e - s).to_pylist()
        if not self._checked:
            self._checked = True
            self.stats["fast_tokenizer"] = self.fast.check(texts[: min(len(texts), 256)])
        lens = None
        tt = time.perf_counter()
        if self.fast.ok:
            lens, flat = self.fast.encode(texts)
            L = self.fast.width(lens)
            names = self.fast.names
            nbytes = len(names) * len(texts) * L * 8
            plan_bytes = int(lens.sum()) * 12 + len(texts) * 24 + 1024   # keep i64 + pos i32 per token; cu, classes, cls rows
            slot, buf = self.in_ring.take(nbytes + plan_bytes)
            host = {}
            for n_, name in enumerate(names):
                host[name] = buf[n_ * len(texts) * L * 8:(n_ + 1) * len(texts) * L * 8].view(torch.int64).view(len(texts), L)
            self.fast.fill(lens, flat, {k: v.numpy() for k, v in host.items()})
        else:  # the tokenizer itself (whatever its kwargs mean), staged through pinned memory all the same
            enc = self.tokenizer(texts, **self.tokenization_kwargs)
            tensors = {k: v for k, v in enc.items()}
            nbytes = sum(v.numel() * v.element_size() + 64 for v in tensors.values())
            slot, buf = self.in_ring.take(nbytes)
            host, off = {}, 0
            for k, v in tensors.items():
                v = v.contiguous()
                nb = v.numel() * v.element_size()
                dst = buf[off:off + nb].view(v.dtype).view(v.shape)
                dst.copy_(v)
                host[k] = dst
                off += (nb + 63) // 64 * 64
        self.stats["tokenize_s"] += time.perf_counter() - tt
        with torch.cuda.device(self.device), torch.cuda.stream(self.side):
            inputs = {k: torch.empty(v.shape, dtype=v.dtype, device=self.device).copy_(v, non_blocking=True) for k, v in host.items()}
            plan = None
            if self.use_plan and lens is not None and "attention_mask" in inputs:
                from .encoders import pack_plan_from_lengths
                cursor = [(nbytes + 63) // 64 * 64]

                def stage(a):  # the plan's host arrays go through the same pinned slot as the token ids
                    nb = a.nbytes
                    dst = buf[cursor[0]:cursor[0] + nb].view(torch.from_numpy(a).dtype).view(a.shape)
                    cursor[0] += (nb + 63) // 64 * 64
                    dst.numpy()[...] = a
                    return dst

                plan = pack_plan_from_lengths(lens, inputs["input_ids"].shape[1], self.device, stage=stage)
            ev = torch.cuda.Event()
            ev.record(self.side)
        self.in_ring.events[slot] = ev
        used = list(inputs.values())
        if plan is not None:
            keep, pos, cu, classes, cls_rows = plan
            used += [keep, pos, cu, cls_rows] + [c[0] for c in classes]
        self.stats["prepare_s"] += time.perf_counter() - t0
        return {"names": texts, "event": ev, "tensors": used, "info": None, "inputs": inputs, "plan": plan}

    # ---- caller's thread -------------------------------------------------------------------------------------------
    def _forward(self, p):
        method = self.model if self.call is None else getattr(self.model, self.call)
        kw = dict(self.forward_kwargs)
        if p["plan"] is not None:
            kw["pack_plan"] = p["plan"]
        return select_output(method(**p["inputs"], **kw), self.output_key)

    def _result(self, batch, found, info):
        batch[self.save_as] = found   # float32 [B, H]
        return batch


def select_output(outputs, output_key):
    """meerqat/ir/embedding.py:227-236: a tensor, or ``outputs[output_key]`` of a dict / list / tuple."""
    if isinstance(outputs, torch.Tensor):
        return outputs
    if isinstance(outputs, (dict, list, tuple)):
        if output_key is None:
            raise ValueError(f"You should set output_key to choose from the model's outputs (got {output_key})")
        return outputs[output_key]
    raise TypeError(f"Invalid type '{type(outputs)}' for model's outputs:\\n{outputs}")


def pipeline_enabled():
    return os.environ.get("MQ_EMBED_PIPELINE", "1") != "0"


def _plain_dataset(dataset, map_kwargs):
    from datasets import Dataset
    return (isinstance(dataset, Dataset) and getattr(dataset, "_indices", None) is None and len(dataset) > 0
            and not map_kwargs.get("num_proc") and map_kwargs.get("batched", True) and not map_kwargs.get("drop_last_batch")
            and not map_kwargs.get("with_rank") and not map_kwargs.get("input_columns") and not map_kwargs.get("with_indices"))


def _map_batch_size(map_kwargs):
    """``Dataset.map``'s batch size, or None when the pipeline does not apply: ``batch_size=None`` means "the whole dataset as one
    batch" there (nothing to pipeline), and a non-positive value is the caller's business."""
    bs = map_kwargs.get("batch_size", 1000)
    if bs is None or isinstance(bs, bool):
        return None
    try:
        bs = int(bs)
    except (TypeError, ValueError):
        return None
    return bs if bs > 0 else None


def _job_batch_size(dataset, map_kwargs, model, key, job_ok, decode_pool=None):
    """The batch size of a job the prefetcher can reproduce ahead of ``Dataset.map`` -- ``job_ok`` (the job's own conditions), the
    pipeline switched on, a CUDA model, a plain ``datasets.Dataset`` walked in order, ``batch[key]`` a string column as it is --
    else None: the caller then maps the serial function, and the decode workers it forked for the pipeline are closed."""
    bs = _map_batch_size(map_kwargs)
    ok = (job_ok and pipeline_enabled() and bs is not None and torch.cuda.is_available() and _plain_dataset(dataset, map_kwargs)
          and _arrow_strings(dataset, key) is not None)
    device = model_device(model) if ok else None
    if device is None or device.type != "cuda":
        if decode_pool is not None:
            decode_pool.close()
        return None
    return bs


def text_pipeline_or_none(dataset, map_kwargs, model=None, tokenizer=None, tokenization_kwargs={}, key="passage",
                          save_as="text_embedding", output_key=None, forward_kwargs={}, layers=None, kb=None, call=None, run=None,
                          qe_predictions_key=None, **other):
    """A :class:`TextEmbedPipeline` for the plain text job (texts = ``batch[key]`` as they are), else None."""
    from .ir.embedding import is_multimodal
    # (the fast tokenizer path truncates on the right like the tokenizer's default; anything else: the serial embed)
    plain = (not other and layers is None and kb is None and run is None and qe_predictions_key is None and tokenizer is not None
             and getattr(tokenizer, "truncation_side", "right") == "right" and isinstance(model, torch.nn.Module)
             and not is_multimodal(model))
    bs = _job_batch_size(dataset, map_kwargs, model, key, plain)
    if bs is None:
        return None
    return TextEmbedPipeline(dataset, model, tokenizer, tokenization_kwargs, key, save_as, output_key, forward_kwargs, call, bs)


# ----------------------------------------------------------------------------------------------------------------------
# images and faces: the decode workers' shared slots
# ----------------------------------------------------------------------------------------------------------------------
def _rgb_plan(sizes):
    """sizes int64 [n, 2] (h, w) -> (geom int64 [n, 3] = (byte offset, h, w), totals int64 [1] = bytes): the decoded RGB images
    back to back at 16-byte aligned offsets, the packing of ``mq_image_plan`` and of ``jpeg.plan_layout``'s host-decoded rows."""
    nbytes = (sizes[:, 0] * sizes[:, 1] * 3 + 15) & ~15
    geom = np.zeros((len(sizes), 3), dtype=np.int64)
    geom[1:, 0] = np.cumsum(nbytes)[:-1]
    geom[:, 1:] = sizes
    return geom, np.array([nbytes.sum()], dtype=np.int64)


def _stage_decode(decode, slot_busy, paths, plan):
    """Decode-slot staging of an image / face batch: sizes -> ``plan(sizes int64 [n, 2]) -> (geom, totals)`` of the readable
    files -> JPEG staging areas (``jpeg.plan_layout``) -> a free slot (``slot_busy``: slot -> (event of the copy that last read
    it, what that copy keeps alive)).  -> (kept, h2d, staging): indices of the readable files, the bytes the batch needs, and
    None when nothing is readable or the batch does not fit a slot, else (slot, geom, totals, layout, offsets, staged)."""
    sizes = decode.sizes(paths)
    kept = [i for i, sz in enumerate(sizes) if sz is not None]
    if not kept:
        return kept, 0, None
    hw = np.array([sizes[i] for i in kept], dtype=np.int64)
    geom, totals = plan(hw)
    jrows = {row: decode.last_jpeg[k] for row, k in enumerate(kept) if k in decode.last_jpeg}
    layout = None
    if jrows:
        from .image import jpeg as dj
        layout = dj.plan_layout(geom, totals, jrows)
        if int(layout["h2d_bytes"]) > decode.slot_bytes:
            # coefficients take 2 bytes per sample: a batch of 4:4:4 files can outgrow a slot its RGB bytes fit -- the workers
            # then decode this batch's files with Pillow, as they do for every other format
            geom, totals = plan(hw)
            jrows, layout = {}, None
    h2d = int(layout["h2d_bytes"] if layout else totals[0])
    if h2d > decode.slot_bytes:
        return kept, h2d, None
    slot = decode.take_slot()
    busy = slot_busy.pop(slot, None)
    if busy is not None:      # the copy that last read this slot (two batches ago) must be over before it is rewritten
        busy[0].synchronize()
    offsets = {k: int(layout["staging"][row] if row in jrows else geom[row, 0]) for row, k in enumerate(kept)}
    return kept, h2d, types.SimpleNamespace(slot=slot, geom=geom, totals=totals, layout=layout, offsets=offsets,
                                            staged={kept[row] for row in jrows})


# ----------------------------------------------------------------------------------------------------------------------
# images
# ----------------------------------------------------------------------------------------------------------------------
class ImageEmbedPipeline(_EncodeJob):
    """The image job (meerqat/image/embedding.py:125-166) with the host stages of batch i + 1 -- file decoding, packing the
    decoded RGB images into one pinned buffer, H2D and the Pillow-exact resize / crop / normalise kernels on a side stream --
    hidden behind the CLIP forward of batch i.  Needs the device-side transform (``transform.on_device``)."""

    def __init__(self, dataset, model, transform, save_as, image_key, call, pool, batch_size, depth=2, decode_procs=None,
                 decode_pool=None):
        self.transform, self.save_as, self.call, self.pool = transform, save_as, call, pool
        self.column = _arrow_strings(dataset, image_key)
        # Decoding.  Default: forked decode PROCESSES that write the RGB bytes straight into a shared page-locked staging slot
        # (viquae_amd/image/decode_pool.py: Pillow's per-file Python holds the GIL, threads stop scaling at ~2x; `processes`
        # of the reference's config sets their number, MQ_IMAGE_DECODE_PROCS the default, 0 disables).  Otherwise the caller's
        # multiprocessing pool (arrays pickled back), or a few threads.
        from .image import decode_pool as dp
        self.decode, self.threads = decode_pool, None
        if self.decode is not None and not hasattr(transform, "run_packed"):
            self.decode.close()
            self.decode = None
        procs = decode_procs if decode_procs is not None else (dp.default_procs() if pool is None else 0)
        if self.decode is None and procs and hasattr(transform, "run_packed") and hasattr(os, "fork"):
            # (created here, the workers are forked from a process that already holds the model: the FIRST device operation
            # after a fork pays for the page-locked memory the process owns -- 4 s with the CLIP weights loaded, 22 s with 2 GB
            # of pinned buffers, measured; image.embedding.dataset_embed therefore forks them before it loads anything)
            try:
                self.decode = dp.DecodePool(procs, dp.slot_bytes(batch_size), n_slots=2)
            except Exception as e:  # noqa: BLE001 - e.g. not enough lockable memory: decode in threads instead
                import warnings
                warnings.warn(f"image decode processes unavailable ({e!r}): decoding in threads")
        if pool is None:
            # also beside the decode processes: a batch whose packed bytes exceed the staging slots (images larger than the slots
            # were sized for) is decoded here, by a few threads -- not one image after the other inside the prefetch thread
            from concurrent.futures import ThreadPoolExecutor
            self.threads = ThreadPoolExecutor(max(1, int(os.environ.get("MQ_IMAGE_DECODE_THREADS", min(8, os.cpu_count() or 1)))))
        self._slot_busy = {}
        decode = (f"{len(self.decode.procs)} processes -> shared pinned staging" if self.decode is not None else
                  "caller's process pool" if pool is not None else f"{self.threads._max_workers} threads")
        super().__init__(dataset, model, image_key, batch_size, {"decode_s": 0.0, "decode": decode}, depth=depth)

    def _prepared(self, names, kept, failed, inputs, ev):
        return {"names": names, "event": ev, "tensors": list(inputs.values()) if inputs else [], "info": (kept, failed),
                "inputs": inputs}

    def _prepare_shared(self, names, t0):
        """Decode workers: sizes -> plan -> decode into the planned offsets of a shared slot -> device-side transform.  None
        when the batch does not fit a slot."""
        from .data import loading
        kept, _, st = _stage_decode(self.decode, self._slot_busy, [str(loading.IMAGE_PATH / n) for n in names], self.transform.plan)
        if not kept:
            return self._prepared(names, kept, set(), None, None)
        if st is None:
            return None  # larger images than the slots were sized for: this batch takes the thread (or caller's pool) path
        failed = self.decode.decode(st.slot, st.offsets, staged=st.staged)
        self.stats["jpeg_scans_decoded_by_workers"] = self.stats.get("jpeg_scans_decoded_by_workers", 0) + len(st.staged)
        self.stats["decode_s"] += time.perf_counter() - t0
        with torch.cuda.device(self.device), torch.cuda.stream(self.side):
            # enqueued only: the DMA of this slot and the resize kernels run while the workers decode the NEXT batch into the
            # other slot
            got = self.transform.run_packed(self.decode.tensors[st.slot], st.geom, st.totals, len(kept), sync=False, jpeg=st.layout)
            ev = torch.cuda.Event()
            ev.record(self.side)
        self._slot_busy[st.slot] = (ev, got.pop("_keep", None))
        return self._prepared(names, kept, failed, dict(got), ev)

    def _prepare(self, j):
        from .data.loading import load_image_array, load_image_batch
        t0 = time.perf_counter()
        s, e = self.bounds[j]
        names = self.column.slice(s, e - s).to_pylist()
        p = self._prepare_shared(names, t0) if self.decode is not None else None
        if p is None:
            if self.threads is not None:
                images = list(self.threads.map(load_image_array, names))
            else:
                images = load_image_batch(names, pool=self.pool, as_arrays=True)
            kept = [i for i, im in enumerate(images) if im is not None]
            self.stats["decode_s"] += time.perf_counter() - t0
            inputs = ev = None
            if kept:
                with torch.cuda.device(self.device), torch.cuda.stream(self.side):
                    inputs = dict(self.transform([images[i] for i in kept], return_tensors="pt"))  # packs, copies, runs its kernels HERE
                    ev = torch.cuda.Event()
                    ev.record(self.side)
            p = self._prepared(names, kept, set(), inputs, ev)
        self.stats["prepare_s"] += time.perf_counter() - t0
        return p

    def _forward(self, p):
        method = self.model if self.call is None else getattr(self.model, self.call)
        out = method(**p["inputs"])
        if not isinstance(out, torch.Tensor):  # transformers >= 5 returns a ModelOutput
            out = out.pooler_output
        return out.reshape(len(p["info"][0]), -1)

    def _result(self, batch, found, info):
        kept, failed = info
        rows = len(batch[self.key])
        if len(kept) == rows and not failed:
            batch[self.save_as] = found   # every image was readable: ONE [B, H] array (Arrow ingests it without a per-row pass)
            return batch
        output = [None] * rows
        if len(failed) == len(kept):
            return output  # (sic) the reference returns the bare list here: meerqat/image/embedding.py:134-135
        for row, k in enumerate(kept):
            if k not in failed:   # a file that opened but did not decode: None, like an unreadable one
                output[k] = found[row]
        batch[self.save_as] = output
        return batch

    def close(self):
        super().close()
        if self.threads is not None:
            self.threads.shutdown(wait=False)
        if self.decode is not None:
            self.decode.close()


def image_pipeline_or_none(dataset, map_kwargs, model=None, transform=None, save_as="image_embedding", image_key="image", call=None,
                           pool=None, decode_procs=None, decode_pool=None, **other):
    """An :class:`ImageEmbedPipeline` when the transform runs on the device, else None; ``decode_pool`` becomes the pipeline's."""
    bs = _job_batch_size(dataset, map_kwargs, model, image_key, not other and getattr(transform, "on_device", False), decode_pool)
    if bs is None:
        return None
    return ImageEmbedPipeline(dataset, model, transform, save_as, image_key, call, pool, bs, decode_procs=decode_procs,
                              decode_pool=decode_pool)


# ----------------------------------------------------------------------------------------------------------------------
# faces
# ----------------------------------------------------------------------------------------------------------------------
class FaceEmbedPipeline(_EncodeJob):
    """The face job (meerqat/image/face_recognition.py:72-112: per batch, load every image that has ``face_landmarks``, align its
    first ``max_n_faces`` faces, run ArcFace) with the host stages of batch i + 1 -- file decoding by the decode workers (JPEG
    files: Huffman scan only, viquae_amd/image/jpeg.py), the 2 x 3 alignment matrices, H2D, the rest of the JPEG decoding and the
    alignment kernel on a side stream -- hidden behind the ArcFace forward of batch i.  Same outputs as the serial
    ``compute_face_embedding`` (the same faces in the same order through the same kernels)."""

    def __init__(self, dataset, model, max_n_faces, image_key, batch_size, decode_pool, depth=2):
        from .image import face_recognition as fr
        self.fr, self.max_n_faces, self.decode = fr, int(max_n_faces), decode_pool
        self.names = _arrow_strings(dataset, image_key)
        self.landmarks = dataset.data.column("face_landmarks")
        self._slot_busy = {}
        self.tform = fr.SimilarityTransform()
        super().__init__(dataset, model, image_key, batch_size,
                         {"decode_s": 0.0, "faces": 0, "decode": f"{len(decode_pool.procs)} processes -> shared pinned staging"},
                         depth=depth)

    def _prepare(self, j):
        from .data import loading
        from .image import jpeg as dj
        from . import _lib
        t0 = time.perf_counter()
        s, e = self.bounds[j]
        names = self.names.slice(s, e - s).to_pylist()
        marks = self.landmarks.slice(s, e - s).to_pylist()
        wanted = [i for i, lm in enumerate(marks) if lm is not None]      # only images with detected faces are loaded (:81-83)
        empty = {"names": names, "event": None, "info": ([], [])}
        if not wanted:
            return empty
        kept, h2d, st = _stage_decode(self.decode, self._slot_busy, [str(loading.IMAGE_PATH / names[i]) for i in wanted], _rgb_plan)
        if not kept:
            return empty
        if st is None:
            raise RuntimeError(f"a batch of {len(kept)} images needs {h2d} bytes of staging, the slots hold {self.decode.slot_bytes}: "
                               "raise MQ_IMAGE_SLOT_KB or set MQ_EMBED_PIPELINE=0")
        # the faces' alignment matrices (Umeyama's estimate per face: ~50 us of small numpy calls each) are the workers' job too
        self.decode.call_start("viquae_amd.image.face_recognition", "face_matrices", {k: (marks[wanted[k]], self.max_n_faces) for k in kept})
        self.decode.decode_start(st.slot, st.offsets, staged=st.staged)
        mats = self.decode.call_finish()
        per_image = [mats[k] for k in kept]
        failed = self.decode.decode_finish()
        self.stats["decode_s"] += time.perf_counter() - t0
        # faces of the images that decoded, in batch order: (row of geom, inverted 2 x 3 matrix)
        images, counts, owner, minv = [], [], [], []
        for row, k in enumerate(kept):
            if k in failed:
                continue
            images.append(wanted[k])
            counts.append(per_image[row][0])
            for m in per_image[row][1]:
                owner.append(row)
                minv.append(m)
        out = dict(empty, info=(images, counts))
        if not owner:
            return out
        lib = _lib.load()
        geom, layout = st.geom, st.layout
        with torch.cuda.device(self.device), torch.cuda.stream(self.side):
            dev = self.device
            src = torch.empty(int(st.totals[0]), dtype=torch.uint8, device=dev)
            src[:h2d].copy_(self.decode.tensors[st.slot][:h2d], non_blocking=True)
            keep = [src]
            if layout is not None:
                keep.append(dj.decode_staged(src, layout["items"], layout["max_blocks"], layout["max_strips"]))
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)  # noqa: E731
            off_d, hw_d = t(geom[:, 0]), t(geom[:, 1:].astype(np.int32).reshape(-1))
            own_d, minv_d = t(np.array(owner, np.int32)), t(np.stack(minv).reshape(-1))
            px = torch.empty((len(owner), 3, self.fr.IMAGE_SIZE, self.fr.IMAGE_SIZE), dtype=torch.float32, device=dev)
            _lib.check(lib.mq_warp_affine_faces_f32(src.data_ptr(), off_d.data_ptr(), hw_d.data_ptr(), own_d.data_ptr(), minv_d.data_ptr(),
                                                    len(owner), self.fr.IMAGE_SIZE, px.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                       "mq_warp_affine_faces_f32")
            ev = torch.cuda.Event()
            ev.record(self.side)
            keep += [off_d, hw_d, own_d, minv_d]
        self._slot_busy[st.slot] = (ev, keep)
        self.stats["prepare_s"] += time.perf_counter() - t0
        self.stats["faces"] += len(owner)
        out.update(event=ev, tensors=[px], inputs=px)
        return out

    def _forward(self, p):
        return self.model(p["inputs"])

    def _result(self, batch, found, info):
        images, counts = info
        output = [None] * len(batch[self.key])
        j = 0
        if sum(counts):   # (a batch without a single face: every entry None, like the reference's early return)
            for at, n_faces in zip(images, counts):
                output[at] = found[j: j + n_faces]
                j += n_faces
        batch["face_embedding"] = output
        return batch

    def close(self):
        super().close()
        self.decode.close()


def face_pipeline_or_none(dataset, map_kwargs, model=None, max_n_faces=1, image_key="image", decode_pool=None, **other):
    """The pipelined face job, or None when it does not apply (then ``compute_face_embedding`` is mapped as the reference does);
    ``decode_pool`` becomes the pipeline's."""
    bs = _job_batch_size(dataset, map_kwargs, model, image_key,
                         not other and decode_pool is not None and "face_landmarks" in dataset.column_names, decode_pool)
    if bs is None:
        return None
    return FaceEmbedPipeline(dataset, model, max_n_faces, image_key, bs, decode_pool)


# ----------------------------------------------------------------------------------------------------------------------
# the job driver of image.embedding.dataset_embed, ir.embedding.dataset_embed and face_recognition.dataset_compute_face_embedding
# ----------------------------------------------------------------------------------------------------------------------
def early_decode_pool(processes, map_kwargs):
    """The decode workers of an image / face job mapped with ``map_kwargs`` (image.decode_pool.early_pool: to be forked before
    the caller loads its model), or None when the pipeline does not apply."""
    bs = _map_batch_size(map_kwargs)
    if bs is None:
        return None
    from .image.decode_pool import early_pool
    return early_pool(processes, bs)


def map_encode_job(job, dataset, map_kwargs, pipe, serial, fn_kwargs, fingerprint=None):
    """``Dataset.map`` of ``pipe.embed``, or of ``serial`` with ``fn_kwargs`` when there is no pipeline; sets
    ``job.last_pipeline_stats``.  The pipelined map is named ``fingerprint()`` unless ``map_kwargs`` names it: ``datasets`` would
    hash the pipeline's bound method by pickling the model's weights and the whole input column."""
    map_kwargs = dict(map_kwargs)
    if pipe is None:
        job.last_pipeline_stats = None
        return dataset.map(serial, batched=True, fn_kwargs=fn_kwargs, **map_kwargs)
    if "new_fingerprint" not in map_kwargs:
        map_kwargs["new_fingerprint"] = fingerprint()
    try:
        return dataset.map(pipe.embed, batched=True, with_indices=True, **map_kwargs)
    finally:
        pipe.close()
        job.last_pipeline_stats = dict(pipe.stats)
