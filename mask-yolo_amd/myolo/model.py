"""
``myolo.model.MaskYOLO`` -- the reference's Python class surface (model.py:761-1391) over the
MI355X-native engine (myolo/engine.py -> libmyolo_hip.so).

Kept: constructor ``MaskYOLO(mode, config, model_dir=None, yolo_pretrain_dir=None,
yolo_trainable=True)`` (model.py:767-785), ``build`` (:787), ``train`` (:943-944), ``compile``
(:1062), ``set_trainable`` (:1120), ``load_weights`` (:1157), ``infer_yolo`` (:1198), ``detect``
(:1238, returns ``[{bboxes, class_ids, confidence_scores, full_masks}]`` :1316-1321),
``decode_masks`` (:1330), and a ``keras_model`` attribute offering ``predict`` / ``summary``.

Deliberate differences: one finalized config object everywhere (the
reference reads the base class from free functions, model.py:25); ``train`` uses every sample of
the dataset unless ``max_samples`` is given (reference hard-codes 50/6, model.py:995,1002);
``detect`` keeps the NMB result (reference overrides it with [109,130], model.py:1306), returns ``bboxes`` in
PIXELS of the input image (x by its width, y by its height; the reference hard-codes ``* 224``, model.py:1307) and
does not mutate ``Config.BATCH_SIZE`` (model.py:1268); ``load_weights`` reads Keras ``.h5`` weight files with a built-in
pure-Python HDF5 reader (no h5py in this image) as well as ``.npz``; ``train`` runs the validation pass Keras' fit_generator runs
(model.py:1053-1054) and keeps the per-epoch numbers in ``self.history``; ``custom_callbacks`` (commented out in the
reference, model.py:1037-1038) are honoured as plain callables ``cb(epoch, logs)``; checkpoints are ``.npz`` keyed by Keras layer names
(and Keras ``.h5`` files are read too); weights are cached by (path, mtime) instead of reloaded per call.
"""
import collections.abc
import contextlib
import datetime
import gc
import os
import queue
import re
import threading
import time

import numpy as np
import torch

from . import detect as D
from . import myolo_utils as mutils
from .engine import Net, layer_table


class _KerasModelShim(object):
    """The two ``keras_model`` methods the reference's scripts call
    (infer_shapes_yolo_model.py:16, train_rice.py:44)."""

    def __init__(self, owner):
        self._o = owner

    def predict(self, inputs, verbose=0):
        o = self._o
        images = inputs[0] if isinstance(inputs, (list, tuple)) else inputs
        x = torch.as_tensor(np.ascontiguousarray(images, np.float32), device=o.net.dev)
        if o.mode == 'yolo':
            return [o.net.predict_yolo(x).cpu().numpy()]
        if o.mode == 'inference':
            return [t.cpu().numpy() for t in o.net.predict(x)]
        raise RuntimeError("predict() on a training-mode model: use train_on_batch()")

    def summary(self):
        lines = ["%-24s %-8s %s" % (n, k, s) for n, k, s, _ in layer_table(self._o.config)]
        txt = "\n".join(lines) + "\ntrainable parameters: %d" % self._o.net.nparam
        print(txt)
        return txt


class StepResult(collections.abc.Mapping):
    """What one training step hands back, without stopping the pipeline.

    Keras' train_on_batch / fit_generator return loss values, not tensors (model.py:1047-1059); rounds 1-3 copied every
    output of the training graph (model.py:899: ~100 MB at config 2) to the host after every step.  Here a step ends with ONE
    small asynchronous device->pinned copy (the loss terms + the per-image positive counts) and an event; the scalar keys
    ('loss', 'yolo_sum_loss', 'mask_loss', 'loss_xy', 'loss_wh', 'loss_conf', 'loss_class', 'recall') wait for that event
    when first read, and the tensor keys ('yolo_output', 'yolo_proposals', 'output_rois', 'myolo_mask', 'target_class_ids',
    'target_mask', 'n_pos', 'feature_map') are downloaded only when indexed (the device tensors stay referenced here, so
    reading them later still gives this step's values).  A read-only Mapping: out['loss'], out.get(...), dict(out) all work.

    Lifetime: while a StepResult is alive it keeps its step's output tensors on the DEVICE (~100 MB at config 2).  Code that collects results
    over many steps should keep numbers, not StepResults: `out["loss"]`, or `out.release()` once the scalars have been read (drops every device
    reference; tensor keys already fetched stay readable, the others then raise), or `out.as_dict()` for a plain, picklable / json-able dict
    of what has been read plus the scalars.  MaskYOLO.train() and train_shapes_stream() do this themselves (they keep the loss of step i-2)."""

    SCALARS = ("loss", "yolo_sum_loss", "mask_loss", "loss_xy", "loss_wh", "loss_conf", "loss_class", "recall")

    def __init__(self, tensors, yolo_terms, mask_terms, loss_weights):
        self._t = dict(tensors)                       # key -> device tensor | None
        self._host = {}
        self._w = loss_weights
        ny = int(yolo_terms.numel())
        self._ny = ny
        self._pin = torch.empty(ny + 2, dtype=torch.float32, pin_memory=True)
        self._pin[:ny].copy_(yolo_terms, non_blocking=True)
        if mask_terms is not None:
            self._pin[ny:ny + 2].copy_(mask_terms, non_blocking=True)
        self._has_mask = mask_terms is not None
        self._ev = torch.cuda.Event()
        self._ev.record(torch.cuda.current_stream())
        self._sc = None

    def _scalars(self):
        if self._sc is None:
            self._ev.synchronize()
            v = self._pin.numpy()
            yt = v[:self._ny]
            m0 = float(v[self._ny]) if self._has_mask else 0.0
            w1, w2 = self._w
            self._sc = dict(yolo_sum_loss=float(yt[0]), mask_loss=m0, loss=float(yt[0] * w1 + m0 * w2) if self._has_mask
                            else float(yt[0] * w1), loss_xy=float(yt[1]), loss_wh=float(yt[2]), loss_conf=float(yt[3]),
                            loss_class=float(yt[4]), recall=float(yt[5]))
        return self._sc

    def ready(self):
        """True when the loss scalars can be read without waiting for the GPU."""
        return self._sc is not None or self._ev.query()

    def __getitem__(self, k):
        if k in self.SCALARS:
            return self._scalars()[k]
        if k not in self._t:
            raise KeyError(k)
        if k not in self._host:
            t = self._t[k]
            self._host[k] = None if t is None else t.cpu().numpy()
        return self._host[k]

    def device(self, k):
        """the device tensor behind a tensor key (no copy)."""
        return self._t[k]

    def release(self):
        """read the scalars (waits for the step's small copy), then drop every device tensor this result holds; returns self.  Tensor keys that
        were downloaded before stay available, the others raise KeyError afterwards."""
        self._scalars()
        self._t = {k: None for k in self._t if k in self._host}
        return self

    def as_dict(self, tensors=()):
        """a plain dict: the eight scalars, every tensor key already downloaded, and the keys named in `tensors` (downloaded now)."""
        d = dict(self._scalars())
        for k in tensors:
            self[k]
        d.update({k: v for k, v in self._host.items()})
        return d

    def __iter__(self):
        return iter(list(self._t.keys()) + list(self.SCALARS))

    def __len__(self):
        return len(self._t) + len(self.SCALARS)


@contextlib.contextmanager
def _gc_parked():
    """the cyclic collector parked for the duration of a training loop (a gen-2 pass over torch's object graph is a
    multi-ms host stall in the middle of the launch sequence); collected once on the way out.  The interpreter's thread switch
    interval is shortened meanwhile: the launch thread and the batch-prefetch thread share the GIL, and the default 5 ms is a
    quarter of a step."""
    import sys
    was = gc.isenabled()
    gc.collect()
    gc.freeze()                   # everything alive now (the model, the dataset) is long-lived: keep it out of the closing collection,
    gc.disable()                  # which then only walks what the loop itself left behind (a full pass cost ~40 ms per epoch of 16 steps)
    sw = sys.getswitchinterval()
    sys.setswitchinterval(min(sw, 0.0005))
    try:
        yield
    finally:
        sys.setswitchinterval(sw)
        if was:
            gc.enable()
        gc.collect()
        gc.unfreeze()


class _Prefetcher(object):
    """Runs `make(i)` for the items of `schedule` one step ahead on a thread (Keras' fit_generator does the same with its
    generator queue, model.py:1055-1058: max_queue_size 3, one worker).  make = BatchGenerator.fill into the engine's pinned
    staging arrays + the asynchronous upload (Net.stage_batch): numpy's copies and the event waits release the GIL, so this
    overlaps the main thread's kernel launches.  close() (train() calls it on every way out: normal end, exception in a step or
    a callback, KeyboardInterrupt) stops the thread and drops what it had staged."""

    def __init__(self, schedule, make, device, depth=2):
        self._q = queue.Queue(maxsize=depth)
        self._err = None
        self._stop = threading.Event()

        def put(item):
            while not self._stop.is_set():
                try:
                    self._q.put(item, timeout=0.05)
                    return True
                except queue.Full:
                    pass
            return False

        def run():
            try:
                if device is not None:
                    torch.cuda.set_device(device)
                for i in schedule:
                    if self._stop.is_set() or not put((i, make(i))):
                        return
            except BaseException as e:                # surfaced in the consumer
                self._err = e
            finally:
                put(None)
        self._th = threading.Thread(target=run, name="myolo-batch-prefetch", daemon=True)
        self._th.start()

    def __iter__(self):
        while True:
            item = self._q.get()
            if item is None:
                if self._err is not None:
                    raise self._err
                return
            yield item

    def close(self, timeout=10.0):
        """stop the thread (it leaves at its next queue operation), drain the queue so that the staged device batches are released, join."""
        self._stop.set()
        try:
            while True:
                self._q.get_nowait()
        except queue.Empty:
            pass
        self._th.join(timeout)
        try:
            while True:
                self._q.get_nowait()
        except queue.Empty:
            pass
        return not self._th.is_alive()


class MaskYOLO(object):
    def __init__(self, mode, config, model_dir=None, yolo_pretrain_dir=None, yolo_trainable=True, device="cuda:0", seed=0):
        assert mode in ['training', 'inference', 'yolo']
        self.mode = mode
        self.config = config.finalize() if hasattr(config, "finalize") else config
        self.model_dir = model_dir
        self.yolo_pretrain_dir = yolo_pretrain_dir
        self.yolo_trainable = yolo_trainable
        self._device, self._seed = device, seed
        self._weights_cache = None
        self._detect_stager = None          # myolo.detect.Stager, made by the first detection call
        self._lr = None
        self._trainable_regex = ".*"
        self._flags = None                  # (key, uint8 [nparam/4] on the device): the recipe path's trainable / decayed byte per group of four
        self._resumed = False               # load_checkpoint ran: train(initial_epoch > 0) may continue from it
        self.global_step = 0                # optimiser steps train() has taken under a recipe (saved by save_checkpoint)
        self.net = self.build(mode=mode, config=self.config)
        self.keras_model = _KerasModelShim(self)
        self.epoch = 0
        # train(): where the launch thread's wall time goes; polygon_batches / segment_batches = the batches that came through
        # Net.stage_segments from a dataset with load_polygons / with load_segments
        self.host_times = {"wait_for_batch_s": 0.0, "launch_step_s": 0.0, "steps": 0, "polygon_batches": 0, "segment_batches": 0}

    # ------------------------------------------------------------------ build
    def build(self, mode, config):
        assert mode in ['training', 'inference', 'yolo']
        w, h = config.IMAGE_SHAPE[:2]
        if w % 32 != 0 or h % 32 != 0:
            raise Exception("Image size must be dividable by 32 to adapt with YOLO framework. "
                            "For example, use 224, 256, 288, 320, 356, ... etc. ")
        # (the reference asserts BACKBONE == "mobilenet", model.py:62; Config.finalize() accepts "mobilenet" and "resnet50" and rejects the rest)
        net = Net(config, device=self._device, seed=self._seed)
        if self.yolo_pretrain_dir is not None:          # model.py:854-868
            self._load_npz_into(net, self.yolo_pretrain_dir, by_name=True)
        return net

    # ------------------------------------------------------------------ weights
    def state_dict(self):
        return self.net.state_dict()

    def load_state_dict(self, sd, strict=True):
        self.net.load_state_dict(sd, strict=strict)

    @staticmethod
    def _load_npz_into(net, filepath, by_name=False, exclude=None):
        """.npz keyed '<keras layer name>/<weight name>', or a Keras .h5 / .hdf5 weight file (keras_io.load_h5_state: the
        reference's checkpoint format, model.py:1024-1027, read without h5py)."""
        if str(filepath).lower().endswith((".h5", ".hdf5")):
            from .keras_io import load_h5_state
            sd = load_h5_state(filepath, exclude=exclude)
        else:
            data = np.load(filepath)
            sd = {}
            for k in data.files:
                layer = k.split("/")[0]
                if exclude and layer in exclude:
                    continue
                sd[k] = data[k]
        net.load_state_dict(sd, strict=not (by_name or exclude))

    def load_weights(self, filepath, by_name=False, exclude=None):
        """model.py:1157-1196: Keras weight files (.h5, as the reference's ModelCheckpoint writes them) or the .npz container
        keyed '<keras layer name>/<weight name>'.  by_name=True loads the layers present in the file and leaves the others;
        exclude drops layers by name (and implies by_name, model.py:1181-1187)."""
        if exclude:
            by_name = True
        key = (os.path.abspath(filepath), os.path.getmtime(filepath), by_name, tuple(exclude or ()))
        if self._weights_cache == key:
            return
        self._load_npz_into(self.net, filepath, by_name=by_name, exclude=exclude)
        self._weights_cache = key

    def save_weights(self, filepath):
        np.savez(filepath, **self.net.state_dict())

    # ------------------------------------------------------------------ recipe: statistics, averaged weights, checkpoints
    def optimizer_stats(self):
        """-> dict(sumsq, norm, scale, skipped, steps): the record the recipe's optimiser pass keeps on the device -- the last
        step's squared gradient norm (float64), its norm and clip scale (float32; scale 0 = that step was skipped), and the counts of skipped and
        of all recipe steps.  Waits for the steps queued so far."""
        return self.net.optimizer_stats()

    @contextlib.contextmanager
    def ema_weights(self):
        """with model.ema_weights(): detect / detect_many / evaluate / save_weights / state_dict see the averaged weights a Recipe(ema=...) keeps.
        The CONTENTS of the live and the averaged buffer are exchanged on the device on entry and again on exit; no tensor is rebound.  BatchNorm
        moving statistics are shared (they are averages already).  Before any recipe step the average is a copy of the weights.  Do not train
        inside the context."""
        self.net.swap_ema()
        try:
            yield self
        finally:
            self.net.swap_ema()

    def save_checkpoint(self, filepath):
        """everything a run needs to go on bit for bit in the optimiser: the state_dict ('state/<name>'), both Adam moments, the EMA if one is
        kept, the optimiser's step count, train()'s global step and the epoch -- one .npz.  See load_checkpoint and train(initial_epoch=...)."""
        net = self.net
        arrays = {"state/" + k: v for k, v in net.state_dict().items()}
        arrays["optim/m"] = net.flat_m.cpu().numpy()
        arrays["optim/v"] = net.flat_v.cpu().numpy()
        if net.flat_ema is not None:
            arrays["optim/ema"] = net.flat_ema.cpu().numpy()
        arrays["optim/adam_t"] = np.int64(net.adam_t)
        arrays["optim/global_step"] = np.int64(self.global_step)
        arrays["optim/epoch"] = np.int64(self.epoch)
        filepath = str(filepath)
        np.savez(filepath if filepath.endswith(".npz") else filepath + ".npz", **arrays)

    def load_checkpoint(self, filepath):
        """restore a save_checkpoint file into this model (same config: the flat layout must match); train(..., initial_epoch=model.epoch)
        then continues the run."""
        net = self.net
        filepath = str(filepath)
        data = np.load(filepath if filepath.endswith(".npz") else filepath + ".npz")
        for key in ("optim/m", "optim/v"):
            if data[key].shape != (net.nparam,):
                raise ValueError("checkpoint %s holds %d values, this model %d: not the same configuration" % (key, data[key].size, net.nparam))
        self.load_state_dict({k[len("state/"):]: data[k] for k in data.files if k.startswith("state/")})
        net.flat_m.copy_(torch.from_numpy(data["optim/m"]))
        net.flat_v.copy_(torch.from_numpy(data["optim/v"]))
        if "optim/ema" in data.files:
            net._ensure_ema().copy_(torch.from_numpy(data["optim/ema"]))
        else:
            net.flat_ema = None
        net.adam_t = int(data["optim/adam_t"])
        self.global_step = int(data["optim/global_step"])
        self.epoch = int(data["optim/epoch"])
        self._weights_cache = None
        self._resumed = True

    # ------------------------------------------------------------------ training
    def set_trainable(self, layer_regex, keras_model=None, indent=0, verbose=1):
        """model.py:1120-1151: layers whose name fully matches the regex are trained; the
        others keep their weights (their gradient is zeroed before Adam)."""
        self._trainable_regex = layer_regex
        mask = torch.zeros_like(self.net.flat_p)
        for k, (off, shp) in self.net.pslots.items():
            if self._layer_trainable(k.split("/")[0]):
                mask[off:off + int(np.prod(shp))] = 1.0
        self._train_mask = None if bool(mask.min() > 0) else mask

    def _layer_trainable(self, layer):
        trainable = bool(re.fullmatch(self._trainable_regex, layer))
        if self.yolo_pretrain_dir is not None and not self.yolo_trainable and not layer.startswith("myolo_mask") \
                and layer != "feature_map":
            trainable = False                      # model.py:867-868
        return trainable

    def _recipe_flags(self):
        """the flags byte of the recipe path (myolo.optim.group_flags) for the current set_trainable regex, on the device; it replaces the mask
        multiply of the plain path: flat_g is not touched"""
        key = (self._trainable_regex, self.yolo_pretrain_dir is not None and not self.yolo_trainable)
        if self._flags is None or self._flags[0] != key:
            from .optim import group_flags
            flags = group_flags(self.net.pslots, self.net.nparam, self._layer_trainable)
            self._flags = (key, torch.from_numpy(flags).to(self.net.dev))
        return self._flags[1]

    def compile(self, learning_rate, momentum):
        """model.py:1062-1118: Adam(lr, 0.9, 0.999, 1e-8); loss = sum of the batch-mean losses
        times LOSS_WEIGHTS.  (momentum is unused by the reference too.)"""
        self._lr = float(learning_rate)
        # the reference instantiates a new keras.optimizers.Adam on every compile() (model.py:1071): fresh moments and
        # step count.  (This is also what keeps frozen layers still: zero gradient AND zero momentum.)
        self.net.flat_m.zero_()
        self.net.flat_v.zero_()
        self.net.adam_t = 0

    def train_on_batch(self, batch, learning_rate=None, *, recipe=None):
        """One optimisation step on a host batch (the six arrays of model.py:896-897) or an already staged device batch.
        Returns a StepResult -- a read-only Mapping of the reference's training outputs (model.py:899) and the loss scalars: scalars from one
        small asynchronous copy (first read waits for the step), tensors downloaded when indexed.  It keeps the step's output tensors on the
        device until dropped: see StepResult (release / as_dict) before collecting results over many steps.
        recipe (keyword only): a myolo.optim.Recipe -- the step's update is Net.recipe_step (clipping, decoupled weight decay, EMA, frozen layers by
        a flags byte) instead of the mask multiply + Net.adam_step; its Schedule is train()'s business, not this method's."""
        if recipe is not None:
            from .optim import check_recipe
            check_recipe(recipe)
        lr = self._lr if learning_rate is None else learning_rate
        if lr is None:
            lr = self.config.LEARNING_RATE
        net = self.net
        db = batch if isinstance(batch, dict) else net.to_device_batch(batch)
        yolo_only = self.mode == 'yolo' or "gt_masks" not in db
        out = net.forward_backward_yolo(db) if yolo_only else net.forward_backward(db)
        if recipe is not None:
            net.recipe_step(lr, recipe, self._recipe_flags())
        else:
            if getattr(self, "_train_mask", None) is not None:
                # data-parallel: the bucketed all-reduces run in place on flat_g on the reducer's stream -- join them BEFORE
                # masking, or RCCL may overwrite zeroed entries / read half-masked data (frozen layers would then move)
                if net.before_optimizer:
                    net.before_optimizer()
                net.flat_g.mul_(self._train_mask)          # torch used as a memory op on a flag vector only
            net.adam_step(lr)
        if yolo_only:
            return StepResult(dict(yolo_output=out["yolo_output"]), out["yolo_terms"], None, out["loss_weights"])
        return self._host_outputs(out)

    @staticmethod
    def _host_outputs(out):
        """-> StepResult: the loss scalars from one small async copy, the graph's tensors on demand."""
        return StepResult({k: out[k] for k in ("yolo_output", "yolo_proposals", "output_rois", "myolo_mask", "target_class_ids",
                                               "target_mask", "n_pos", "feature_map")},
                          out["yolo_terms"], out["mask_terms"], out["loss_weights"])

    def _data_parallel(self):
        """(rank, world): when torch.distributed is initialised with more than one rank (myolo.dist.init_from_env under
        torchrun), hook the bucketed gradient all-reduce into the engine once and shard the work by rank -- every rank holds
        the same seeded weights, trains on its own BATCH_SIZE images per step (global batch = world * BATCH_SIZE) and applies
        the same averaged update.  Single process: (0, 1), nothing attached."""
        import torch.distributed as tdist
        if not (tdist.is_available() and tdist.is_initialized()) or tdist.get_world_size() == 1:
            return 0, 1
        if getattr(self, "_reducer", None) is None:
            from .dist import GradReducer
            self._reducer = GradReducer(self.net.flat_g, self.net.bucket_ranges, stream=self.net._copy_stream).attach(self.net)
        return tdist.get_rank(), tdist.get_world_size()

    def evaluate_on_batch(self, batch):
        """Forward-only losses of one host batch in Keras' test phase (every BatchNormalization on its moving statistics):
        what fit_generator's validation pass computes per batch (model.py:1053-1054).  No state is changed."""
        net = self.net
        db = batch if isinstance(batch, dict) else net.to_device_batch(batch)
        out = net.forward_loss(db)
        yt = out["yolo_terms"].cpu().numpy()
        mt = out["mask_terms"].cpu().numpy()
        w1, w2 = out["loss_weights"]
        return dict(loss=float(yt[0] * w1 + mt[0] * w2), yolo_sum_loss=float(yt[0]), mask_loss=float(mt[0]),
                    loss_xy=float(yt[1]), loss_wh=float(yt[2]), loss_conf=float(yt[3]), loss_class=float(yt[4]), recall=float(yt[5]))

    def train(self, train_dataset, val_dataset, learning_rate, epochs, layers,
              augmentation=None, custom_callbacks=None, no_augmentation_sources=None, max_samples=None, verbose=1, shuffle_seed=0,
              device_polygons=True, mosaic=None, *, recipe=None, initial_epoch=0, photometric=None, copy_paste=None):
        """model.py:943-1060.  Returns the list of per-epoch mean training losses; ``self.history`` holds
        {"loss": [...], "val_loss": [...]} like the Keras History the reference's fit_generator produces.
        shuffle_seed: the generators' one-off shuffle (myolo_utils.py:711-712) draws from RandomState(shuffle_seed) -- the
        same permutation on every data-parallel rank, so that dp_batch_indices really hands out disjoint samples; None =
        the global numpy generator, as the reference (single process only).
        device_polygons: a train_dataset that has load_polygons (myolo.via.VIADataset) is never asked for a mask: its outlines go to the device
        as one-part segments and are filled there, in front of the device augmenter (identity rows with augmentation=None) -- DESIGN.md sections 13
        and 18.  An outline that
        fills no pixel is dropped on the device, AFTER the sub-sampling to TRUE_BOX_BUFFER instances (the host route drops it before).
        A train_dataset that has load_segments (myolo.coco.COCODataset) goes the same way under the same flag -- "annotations decoded on the
        device": its polygon parts and run-length codes are decoded by myolo_segment_masks.
        False, or a dataset with neither: load_mask and the host route.  Validation batches always use load_mask.
        mosaic: a myolo.augment.Mosaic -- every training sample it picks is cut into four tiles that show the sample and three others of the same
        batch, on the device, on every route, with or without `augmentation` (without: identity rows; on the host route the
        device augmenter then runs all the same).  Samples whose source is in no_augmentation_sources are neither mosaicked nor used as partners;
        validation batches never are.
        copy_paste (keyword only): a myolo.augment.CopyPaste -- every training sample it picks receives instances of another sample of its batch,
        pasted on the device after both have been augmented / mosaicked, on every route, with or without `augmentation`
        and `mosaic`.  Samples whose source is in no_augmentation_sources neither receive nor donate; validation batches are never pasted.
        photometric (keyword only): a myolo.augment.Photometric -- hue, saturation, contrast, Gaussian blur and noise on the pixels of every
        training sample it picks, on the device, after every other stage, on every route, with or without `augmentation`,
        `mosaic` and `copy_paste`; masks, boxes and targets are untouched.  Samples whose source is in no_augmentation_sources and validation
        batches are left as they are.
        recipe (keyword only): a myolo.optim.Recipe -- gradient clipping, decoupled weight decay, an EMA of the weights and a learning-rate
        Schedule, all in the optimiser pass on the device.  Step k of the run (counted over all epochs) is taken at
        schedule.lr_at(k, epochs * steps per epoch, learning_rate).  The per-epoch logs and self.history gain "lr" (the epoch's last step),
        "grad_norm" (that step's gradient norm before clipping) and "skipped_steps" (steps the device skipped for a non-finite norm, so far), from
        one small copy of the device's record at the epoch end; with recipe.ema and a model_dir, saved_model_<stamp>_ema.npz holds the averaged
        weights beside the epoch's checkpoint.  None: the plain Adam path, as ever.
        initial_epoch (keyword only): continue a run restored by load_checkpoint at this epoch: the moments, the step count and the EMA are kept
        and the schedule goes on at step initial_epoch * steps per epoch.  Without a loaded checkpoint it must be 0."""
        if recipe is not None:
            from .optim import check_recipe
            check_recipe(recipe)
        initial_epoch = int(initial_epoch)
        if initial_epoch < 0 or initial_epoch > epochs:
            raise ValueError("initial_epoch must be in [0, epochs], got %r" % (initial_epoch,))
        if initial_epoch and not self._resumed:
            raise ValueError("initial_epoch > 0 continues a run restored by load_checkpoint(); none was loaded")
        layer_regex = {"all": ".*"}
        if layers in layer_regex:
            layers = layer_regex[layers]
        cfg = self.config
        if augmentation is not None:
            from .augment import Augmentation
            if not isinstance(augmentation, Augmentation):
                raise TypeError("augmentation must be a myolo.augment.Augmentation (the warp runs on the device; imgaug objects are not taken), "
                                "got %r" % type(augmentation).__name__)
        if mosaic is not None:
            from .augment import Mosaic
            if not isinstance(mosaic, Mosaic):
                raise TypeError("mosaic must be a myolo.augment.Mosaic, got %r" % type(mosaic).__name__)
        if copy_paste is not None:
            from .augment import CopyPaste
            if not isinstance(copy_paste, CopyPaste):
                raise TypeError("copy_paste must be a myolo.augment.CopyPaste, got %r" % type(copy_paste).__name__)
        if photometric is not None:
            from .augment import Photometric
            if not isinstance(photometric, Photometric):
                raise TypeError("photometric must be a myolo.augment.Photometric, got %r" % type(photometric).__name__)
        device_augmenter = augmentation is not None or mosaic is not None or copy_paste is not None or photometric is not None

        def collect(ds, tag=False):
            ids = list(ds.image_ids)
            if max_samples is not None:
                ids = ids[:max_samples]
            info = [list(mutils.load_image_gt(ds, cfg, i, use_mini_mask=cfg.USE_MINI_MASK)) for i in ids]
            if tag:        # the augmented path keys a sample's parameters by its dataset image id: the generator shuffles these rows
                for inst, i in zip(info, ids):
                    inst.append(int(i))
            return info

        polygon_route = bool(device_polygons) and hasattr(train_dataset, "load_polygons")
        segment_route = bool(device_polygons) and not polygon_route and hasattr(train_dataset, "load_segments")
        if polygon_route or segment_route:
            train_info = self._collect_segments(train_dataset, max_samples, load="load_polygons" if polygon_route else "load_segments")
        else:
            train_info = collect(train_dataset, tag=device_augmenter)
        val_info = collect(val_dataset) if val_dataset is not None else []
        mode = self.mode if self.mode in ('yolo', 'training') else 'training'
        rank, world = self._data_parallel()
        if world > 1 and shuffle_seed is None:
            raise ValueError("data-parallel train() needs a shuffle_seed: every rank must hold the same permutation")
        rng = None if shuffle_seed is None else np.random.RandomState(shuffle_seed)
        train_gen = mutils.BatchGenerator(train_info, cfg, mode=mode, shuffle=True, jitter=False, norm=True, rng=rng)
        val_gen = mutils.BatchGenerator(val_info, cfg, mode=mode, shuffle=True, jitter=False, norm=True, rng=rng) if val_info else None
        self.set_trainable(layers)
        if initial_epoch:
            self._lr = float(learning_rate)            # a resumed run keeps its moments and step count
        else:
            self.compile(learning_rate, cfg.LEARNING_MOMENTUM)
        from .dist import dp_batch_indices
        schedule = dp_batch_indices(len(train_info), cfg.BATCH_SIZE, rank, world, len(train_gen))   # raises if < one batch
        history = []
        self.history = {"loss": [], "val_loss": []}
        if recipe is not None:
            self.history.update(lr=[], grad_norm=[], skipped_steps=[])
        n_steps = len(train_gen)
        total_steps = epochs * len(schedule)

        bytes_ok = bool(train_info) and all(inst[0].dtype == np.uint8 for inst in train_info)

        def make(i):                                   # runs on the prefetch thread, one batch ahead of the step
            # BatchGenerator.__getitem__'s arrays (the wrapped last batch is full-size, myolo_utils.py:730-735) encoded straight into
            # the engine's pinned staging buffers; images travel as bytes and are normalised on the device
            lo, hi = train_gen.batch_bounds(i)
            return self.net.stage_batch(lambda arrays: train_gen.fill(i, arrays), hi - lo, yolo=(mode == 'yolo'), u8_images=bytes_ok)

        def report(ep, i, out):
            losses.append(out["loss"])
            if verbose:
                print("epoch %d step %d/%d loss %.4f (yolo %.4f mask %.4f recall %.3f)" %
                      (ep + 1, i + 1, n_steps, out["loss"], out["yolo_sum_loss"], out["mask_loss"], out["recall"]))

        make_item = lambda it: make(it[1])             # noqa: E731
        if polygon_route or segment_route:
            make_item = self._segment_batches(augmentation, no_augmentation_sources, train_dataset, train_gen, mode, mosaic,
                                              counter="polygon_batches" if polygon_route else "segment_batches", copy_paste=copy_paste,
                                              photometric=photometric)
        elif device_augmenter:
            make_item = self._augmented_batches(augmentation, no_augmentation_sources, train_dataset, train_gen, mode, mosaic, copy_paste=copy_paste,
                                                photometric=photometric)

        # ONE prefetcher for the whole run (Keras' generator queue also keeps running across epoch ends): the first batches of epoch e+1
        # are encoded and uploaded while epoch e finishes
        prefetch = _Prefetcher([(e, i) for e in range(initial_epoch, epochs) for i in schedule], make_item, self.net.dev)
        stream = iter(prefetch)
        try:
            with _gc_parked():                          # for the whole run: a full collection at every epoch end cost ~50 ms per epoch
                for ep in range(initial_epoch, epochs):
                    losses = []
                    pending = None
                    for k in range(len(schedule)):
                        t0 = time.perf_counter()
                        (_, i), db = next(stream)
                        t1 = time.perf_counter()
                        if recipe is None:
                            out = self.train_on_batch(db)
                        else:
                            self.global_step = ep * len(schedule) + k
                            lr_now = recipe.lr_at(self.global_step, total_steps, learning_rate)
                            out = self.train_on_batch(db, lr_now, recipe=recipe)
                            self.global_step += 1
                        self.host_times["wait_for_batch_s"] += t1 - t0      # the launch thread blocked on the prefetch queue
                        self.host_times["launch_step_s"] += time.perf_counter() - t1
                        self.host_times["steps"] += 1
                        if pending is not None:            # step i-1's numbers are read once step i is queued behind it: the
                            report(ep, *pending)           # host never waits for the step it has just launched
                        pending = (i, out)
                    if pending is not None:
                        report(ep, *pending)
                    gc.collect(0)                          # the young generation only (cheap): what this epoch's steps left behind
                    history.append(float(np.mean(losses)))
                    logs = {"loss": history[-1]}
                    if recipe is not None:                 # one small copy of the device's record; the epoch's last step has been waited for above
                        st = self.optimizer_stats()
                        logs.update(lr=lr_now, grad_norm=st["norm"], skipped_steps=st["skipped"])
                        for key in ("lr", "grad_norm", "skipped_steps"):
                            self.history[key].append(logs[key])
                        self.epoch = max(self.epoch, ep + 1)    # what a save_checkpoint from a callback records
                    if val_gen is not None and len(val_info) >= cfg.BATCH_SIZE:
                        # validation_data=val_generator, validation_steps=len(val_generator) (model.py:1053-1054): forward only, BN on
                        # moving statistics, batch-mean of the total loss.  Every rank evaluates the same (small) set.
                        vl = [self.evaluate_on_batch(val_gen[j][0])["loss"] for j in range(len(val_gen))]
                        logs["val_loss"] = float(np.mean(vl))
                        if verbose:
                            print("epoch %d val_loss %.4f" % (ep + 1, logs["val_loss"]))
                    self.history["loss"].append(logs["loss"])
                    self.history["val_loss"].append(logs.get("val_loss", float("nan")))
                    if self.model_dir and rank == 0:
                        os.makedirs(self.model_dir, exist_ok=True)
                        stamp = datetime.datetime.now().strftime('%b%d-%H-%M')
                        self.save_weights(os.path.join(self.model_dir, 'saved_model_' + stamp + '.npz'))   # model.py:1026
                        if recipe is not None and recipe.ema is not None:
                            with self.ema_weights():
                                self.save_weights(os.path.join(self.model_dir, 'saved_model_' + stamp + '_ema.npz'))
                    for cb in (custom_callbacks or []):
                        (cb.on_epoch_end if hasattr(cb, "on_epoch_end") else cb)(ep, dict(logs))
            for _ in stream:                               # (drains the prefetch thread: nothing is left when every epoch ran)
                pass
        finally:
            prefetch.close()       # every way out (a failing step or callback, Ctrl-C): no thread is left staging into the engine's ring

        self.epoch = max(self.epoch, epochs)
        return history

    def augmentation_rows(self, augmentation, no_augmentation_sources, dataset, epoch, image_ids):
        """-> float64 [n,8]: the parameter rows train() hands the device augmenter for these dataset image ids in this epoch -- keyed by image id
        and epoch (never by position after the shuffle), the identity for a sample whose source is in no_augmentation_sources."""
        from .augment import IDENTITY_ROW
        H, W = self.config.IMAGE_SHAPE[0], self.config.IMAGE_SHAPE[1]
        skip = set(no_augmentation_sources or [])
        rows = np.empty((len(image_ids), 8), np.float64)
        for k, i in enumerate(image_ids):
            plain = bool(skip) and dataset.image_info[i]['source'] in skip
            rows[k] = IDENTITY_ROW if plain else augmentation.params(epoch, i, H, W)
        return rows

    def _row_of(self, augmentation, no_augmentation_sources, dataset, epoch):
        """-> row_of(sample) for the generators' fill functions: the sample's parameter row in this epoch, the identity with augmentation=None"""
        from .augment import IDENTITY_ROW
        if augmentation is None:
            return lambda inst: IDENTITY_ROW
        return lambda inst: self.augmentation_rows(augmentation, no_augmentation_sources, dataset, epoch, [inst[4]])[0]

    def mosaic_tables(self, mosaic, no_augmentation_sources, dataset, epoch, image_ids):
        """-> (src [n,4], tiles [n,4,6], centre [n,2]): the plan train() draws for a batch that holds these dataset image ids, in this order, in this
        epoch (Mosaic.plan).  A sample whose source is in no_augmentation_sources is neither mosaicked nor a partner."""
        skip = set(no_augmentation_sources or [])
        eligible = [k for k, i in enumerate(image_ids) if not (skip and dataset.image_info[i]['source'] in skip)]
        return mosaic.plan(epoch, image_ids, self.config.IMAGE_SHAPE[0], self.config.IMAGE_SHAPE[1], eligible)

    def _with_mosaic(self, mosaic, no_augmentation_sources, dataset, gen, epoch, i, fill):
        """fill(arrays) -> a fill for the same batch with the three mosaic tables staged behind the parameter rows (Net._mosaic_spec): the plan of the
        batch's image ids, composed with the rows `fill` wrote, checked before the upload is queued.  mosaic=None: `fill` itself."""
        if mosaic is None:
            return fill
        from .augment import check_mosaic_tables
        lo, hi = gen.batch_bounds(i)
        src, tiles, centre = self.mosaic_tables(mosaic, no_augmentation_sources, dataset, epoch, [inst[4] for inst in gen.all_info[lo:hi]])
        check_mosaic_tables(src, centre, hi - lo, self.config.IMAGE_SHAPE[0], self.config.IMAGE_SHAPE[1])

        def both(arrays):
            fill(arrays[:-3])
            arrays[-3][...], arrays[-2][...], arrays[-1][...] = src, mosaic.compose(tiles, src, arrays[-4]), centre
            return arrays
        return both

    def paste_tables(self, copy_paste, no_augmentation_sources, dataset, epoch, image_ids):
        """-> (donor [n], select [n]): the plan train() draws for a batch that holds these dataset image ids, in this order, in this epoch
        (CopyPaste.plan).  A sample whose source is in no_augmentation_sources neither receives nor donates."""
        skip = set(no_augmentation_sources or [])
        eligible = [k for k, i in enumerate(image_ids) if not (skip and dataset.image_info[i]['source'] in skip)]
        return copy_paste.plan(epoch, image_ids, self.config.TRUE_BOX_BUFFER, eligible)

    def _with_paste(self, copy_paste, no_augmentation_sources, dataset, gen, epoch, i, fill):
        """fill(arrays) -> a fill for the same batch with the two copy-paste tables staged last (Net._paste_spec): the plan of the batch's image
        ids, checked before the upload is queued.  copy_paste=None: `fill` itself."""
        if copy_paste is None:
            return fill
        from .augment import check_paste_tables
        lo, hi = gen.batch_bounds(i)
        donor, select = self.paste_tables(copy_paste, no_augmentation_sources, dataset, epoch, [inst[4] for inst in gen.all_info[lo:hi]])
        check_paste_tables(donor, select, hi - lo, self.config.TRUE_BOX_BUFFER)

        def both(arrays):
            fill(arrays[:-2])
            arrays[-2][...], arrays[-1][...] = donor, select
            return arrays
        return both

    def photometric_rows(self, photometric, no_augmentation_sources, dataset, epoch, image_ids):
        """-> float64 [n,32]: the rows train() hands the device augmenter's last stage for these dataset image ids in this epoch (Photometric.row),
        keyed by image id and epoch, the identity for a sample whose source is in no_augmentation_sources."""
        skip = set(no_augmentation_sources or [])
        rows = np.empty((len(image_ids), 32), np.float64)
        rs = np.random.RandomState(0)          # re-seeded per sample, as in Mosaic.plan
        for k, i in enumerate(image_ids):
            plain = bool(skip) and dataset.image_info[i]['source'] in skip
            rows[k] = photometric.identity() if plain else photometric.row(epoch, i, rs)
        return rows

    def _with_photo(self, photometric, no_augmentation_sources, dataset, gen, epoch, i, fill):
        """fill(arrays) -> a fill for the same batch with the photometric rows staged last of all (Net._photo_spec): the rows of the batch's image
        ids, checked before the upload is queued.  photometric=None: `fill` itself."""
        if photometric is None:
            return fill
        from .augment import check_photo_rows
        lo, hi = gen.batch_bounds(i)
        rows = self.photometric_rows(photometric, no_augmentation_sources, dataset, epoch, [inst[4] for inst in gen.all_info[lo:hi]])
        check_photo_rows(rows, hi - lo)

        def both(arrays):
            fill(arrays[:-1])
            arrays[-1][...] = rows
            return arrays
        return both

    def _augmented_batches(self, augmentation, no_augmentation_sources, dataset, gen, mode, mosaic=None, copy_paste=None, photometric=None):
        """-> make((epoch, batch index)) for train()'s prefetch thread: raw bytes, un-augmented masks, class ids and parameter rows go up through the
        engine's staging ring, and the device augmenter runs behind the copies on the copy stream, under the previous step."""
        from .augment import DeviceAugmenter
        if not all(inst[0].dtype == np.uint8 for inst in gen.all_info):
            raise ValueError("train(augmentation=...) and train(mosaic=...) need uint8 images")
        aug = DeviceAugmenter(self.config, self.net.dev, cval=0.0 if augmentation is None else augmentation.cval)

        def make(it):
            epoch, i = it
            lo, hi = gen.batch_bounds(i)
            row_of = self._row_of(augmentation, no_augmentation_sources, dataset, epoch)
            fill = self._with_mosaic(mosaic, no_augmentation_sources, dataset, gen, epoch, i, lambda arrays: gen.fill_raw(i, arrays, row_of))
            fill = self._with_paste(copy_paste, no_augmentation_sources, dataset, gen, epoch, i, fill)
            fill = self._with_photo(photometric, no_augmentation_sources, dataset, gen, epoch, i, fill)
            return self.net.stage_augmented(fill, hi - lo, aug, yolo=(mode == 'yolo'), mosaic=mosaic is not None, copy_paste=copy_paste is not None,
                                            photometric=photometric is not None, photo_radius=photometric.max_radius if photometric else 0)
        return make

    def _collect_segments(self, dataset, max_samples=None, first=None, load="load_segments"):
        """train()'s and evaluate()'s sample list on the device route: per image [image resized to the network frame uint8, class ids int32 [n],
        segments (a list of float64 [k,2] (row, col) parts in source-image pixels, or a run-length code {"size", "counts"}), (source-row table int32
        [H], source-column table int32 [W]), dataset image id, source image height].  load_image_gt without load_mask: the tables name the source
        pixel resize_mask would read for every pixel of the network frame.  load: "load_segments" (myolo.coco), or "load_polygons" (myolo.via):
        every outline is taken as a one-part segment.  first: keep an image's first `first` segments only (evaluate())."""
        cfg = self.config
        if cfg.USE_MINI_MASK:
            raise NotImplementedError("mini-masks are outside the hot path")
        H, W = cfg.IMAGE_SHAPE[0], cfg.IMAGE_SHAPE[1]
        ids = list(dataset.image_ids)
        if max_samples is not None:
            ids = ids[:max_samples]
        info = []
        for i in ids:
            image = dataset.load_image(i)
            segs, class_ids = mutils.segments_of(dataset, i, load)
            class_ids = np.asarray(class_ids, dtype=np.int32)
            h, w = image.shape[:2]
            if load == "load_polygons":
                if len(segs) != class_ids.shape[0] or any(p.ndim != 2 or p.shape[1] != 2 or p.shape[0] == 0 or not np.isfinite(p).all() for p, in segs):
                    raise ValueError("load_polygons(%r): need one finite [k,2] (row, col) array with k >= 1 per class id" % (i,))
            elif len(segs) != class_ids.shape[0]:
                raise ValueError("load_segments(%r): %d segments but %d class ids" % (i, len(segs), class_ids.shape[0]))
            for s in segs:
                if isinstance(s, dict):
                    c = np.asarray(s["counts"])
                    ok = list(s["size"]) == [h, w] and h * w < 1 << 31 and c.ndim == 1 and c.size > 0 and (c >= 0).all() and int(c.sum()) == h * w
                else:
                    ok = all(isinstance(p, np.ndarray) and p.dtype == np.float64 and p.ndim == 2 and p.shape[1] == 2 and p.shape[0] > 0 and
                             np.isfinite(p).all() for p in s)
                if not ok:
                    raise ValueError("load_segments(%r): a segment is a list of finite float64 [k,2] (row, col) parts with k >= 1, or a run-length "
                                     "code whose counts are >= 0 and sum to the %d x %d image" % (i, h, w))
            scale = [1, 1]
            if [h, w] != [H, W]:
                image, scale = mutils.resize_image(image, cfg.IMAGE_SHAPE)
            rows, cols = mutils.mask_index_tables(h, w, scale)
            if rows.shape[0] != H or cols.shape[0] != W:
                raise ValueError("image %r: %d x %d does not resize to the %d x %d network frame" % (i, h, w, H, W))
            if first is not None:
                segs, class_ids = list(segs)[:first], class_ids[:first]
            info.append([image, class_ids, list(segs), (rows.astype(np.int32), cols.astype(np.int32)), int(i), int(h)])
        return info

    def _segment_batches(self, augmentation, no_augmentation_sources, dataset, gen, mode, mosaic=None, counter="segment_batches", copy_paste=None,
                         photometric=None):
        """-> make((epoch, batch index)) for train()'s prefetch thread on the device route: image bytes, segments, class ids, index tables and
        parameter rows go up through the engine's staging ring; Net.stage_segments decodes the segments behind the copies on the copy stream, then
        the device augmenter runs.  counter: the key of host_times that counts the batches ("polygon_batches" for a dataset with load_polygons)."""
        from .augment import DeviceAugmenter
        if not all(inst[0].dtype == np.uint8 for inst in gen.all_info):
            raise ValueError("train() on a dataset with load_%ss needs uint8 images (or device_polygons=False)" % counter[:-len("_batches")])
        aug = DeviceAugmenter(self.config, self.net.dev, cval=0.0 if augmentation is None else augmentation.cval)

        def make(it):
            epoch, i = it
            lo, hi = gen.batch_bounds(i)
            fill, n_verts, n_parts, n_bounds = gen.segment_batch(i, self._row_of(augmentation, no_augmentation_sources, dataset, epoch))
            fill = self._with_mosaic(mosaic, no_augmentation_sources, dataset, gen, epoch, i, fill)
            fill = self._with_paste(copy_paste, no_augmentation_sources, dataset, gen, epoch, i, fill)
            fill = self._with_photo(photometric, no_augmentation_sources, dataset, gen, epoch, i, fill)
            db = self.net.stage_segments(fill, hi - lo, aug, yolo=(mode == 'yolo'), n_verts=n_verts, n_parts=n_parts, n_bounds=n_bounds,
                                         mosaic=mosaic is not None, copy_paste=copy_paste is not None, photometric=photometric is not None,
                                         photo_radius=photometric.max_radius if photometric else 0)
            self.host_times[counter] += 1
            return db
        return make

    def train_shapes_stream(self, steps, learning_rate=None, seed=1234, start_index=0, verbose=0):
        """Train on the endless synthetic Shapes stream with the inputs produced ON THE DEVICE
        (myolo.shapes.ShapesProducer): image g of the stream is bit-identical to what
        ShapesDataset/load_image_gt/BatchGenerator would feed, without the Python rasteriser in the loop."""
        from .shapes import ShapesProducer
        cfg = self.config
        prod = ShapesProducer(cfg, seed=seed, device=self._device)
        self.set_trainable(".*")
        self.compile(cfg.LEARNING_RATE if learning_rate is None else learning_rate, cfg.LEARNING_MOMENTUM)
        rank, world = self._data_parallel()          # rank r takes images [r*B, (r+1)*B) of each global batch of world*B
        results = []
        import torch
        side = self.net._copy_stream                 # batch i+1 is produced there while step i runs (its kernels are a few hundred microseconds)

        def produce(i):
            lo = start_index + (i * world + rank) * cfg.BATCH_SIZE
            return prod.batch(list(range(lo, lo + cfg.BATCH_SIZE)), stream=side, consumer=torch.cuda.current_stream())
        with _gc_parked():
            nxt = produce(0) if steps else None
            for i in range(steps):
                cur, nxt = nxt, (produce(i + 1) if i + 1 < steps else None)
                results.append(self.train_on_batch(cur))
                if verbose and i:
                    print("step %d loss %.4f" % (i, results[i - 1]["loss"]))      # one step behind: no wait on the step in flight
                if i >= 2:
                    results[i - 2] = results[i - 2]["loss"]                          # long finished: keep the number, drop the tensors
        losses = [r if isinstance(r, float) else r["loss"] for r in results]
        if verbose and steps:
            print("step %d loss %.4f" % (steps, losses[-1]))
        return losses

    # ------------------------------------------------------------------ inference
    def infer_yolo(self, image, weights_dir=None, save_path=None, display=False):
        """model.py:1198-1236 without the plotting: returns the decoded BoundBox list."""
        cfg = self.config
        assert list(image.shape) == list(cfg.IMAGE_SHAPE)
        assert image.dtype == 'uint8'
        assert self.mode == 'yolo'
        if weights_dir is not None:
            self.load_weights(weights_dir)
        normed = np.expand_dims(image / 255., axis=0)
        netout = self.keras_model.predict([normed])[0]
        return mutils.decode_one_yolo_output(netout[0], anchors=cfg.ANCHORS, nms_threshold=0.3, obj_threshold=0.35,
                                             nb_class=cfg.NUM_CLASSES)

    EVAL_SLOTS = D.SLOTS       # detect() keeps at most the top 10 detections of an image (the drivers below run the three pieces of myolo/detect.py)

    def _stager(self):
        if self._detect_stager is None:
            self._detect_stager = D.Stager(self.net)
        return self._detect_stager

    def _select(self, det_h, cs_threshold):
        """detect()'s selection of one image (detect.select): -> keep, nmb, boxes, scores, class_ids; the selected rows of det_h [R,6] are keep[nmb]"""
        return D.select(det_h, cs_threshold, self.config.IMAGE_SHAPE)

    def _frames(self, images, mask_frame):
        return [im.shape if mask_frame == "image" else self.config.IMAGE_SHAPE for im in images]

    def detect(self, image, weights_dir=None, save_path='./img_results/', cs_threshold=0.35, display=False, mask_frame="image",
               mask_format="dense", render=False, *, max_detections=None, measure=False):
        """model.py:1238-1328.  Returns [ {bboxes, class_ids, confidence_scores, full_masks} ].  An image of another size than config.IMAGE_SHAPE
        is resized to it on the device (Net.resize_to_frame: myolo_utils.resize_image's result, bit for bit) and reported in
        the frame mask_frame names: "image" -- bboxes in pixels of the image given, full_masks [h,w,n] pasted at that size -- or "network" --
        both in the IMAGE_SHAPE frame, as detect(resize_image(image, IMAGE_SHAPE)[0]) gives them.
        mask_format="rle": instead of full_masks the dict has rle_masks, a list of COCO run-length dicts {"size": [h, w], "counts": int64 array}
        (myolo/rle.py) in the order of class_ids, size = the frame mask_frame names; rle.decode of each is the full_masks plane bit for bit.  The
        masks are encoded on the device (Net.rle_masks) and no dense mask is written or downloaded.  Not supported together
        with config.DETECT_MASKS_FOR_SELECTED_ONLY (ValueError).
        mask_format="polygon": instead of full_masks the dict has polygons, a list in the order of class_ids of each instance's closed loops: int32
        [n,2] (X, Y) arrays in lattice corner coordinates of the frame mask_frame names (pixel (y, x) is the square [x, x+1] x [y, y+1]), outer
        loops clockwise on screen, holes the other way, in the order of myolo/contour.py -- contour.trace of the full_masks plane integer for
        integer.  The masks are traced on the device (Net.contour_masks) and no dense mask is written or downloaded;
        myolo.via.via_annotations and myolo.rle.coco_results write the results out.  Not supported together with
        config.DETECT_MASKS_FOR_SELECTED_ONLY (ValueError).  Any other mask_format raises ValueError.
        render=True: the dict gains "rendered", uint8 [h,w,3]: the overlay the reference's detect() draws (visualize.display_instances without the
        captions) over the image given -- the masks blended in, their outlines, the dashed boxes, instance i of class_ids in colour i of
        render.instance_colors(len(class_ids)) -- drawn on the device from the uploaded bytes (Net.render_instances); with a
        save_path that is not None it is also written to save_path/InferMaskYOLO-0.png (the directory is created).
        ValueError with mask_frame="network" for an image of another size than IMAGE_SHAPE (the canvas is the image given) and with
        config.DETECT_MASKS_FOR_SELECTED_ONLY.  Without render, save_path and display are ignored.
        max_detections=K, an int in 1 .. 128 (keyword only): up to K instances per image instead of ten, selected on the device
        (Net.select_detections, DESIGN.md section 23: detect.select with its 10 replaced by K, every decision bit for bit the host's; K = 10 gives
        the results of None wherever no two candidates tie in score -- among equal scores the device takes the higher row first, a stable
        argsort reversed, where the host's default argsort promises no order).  ValueError for any other value, with config.DETECT_MASKS_FOR_SELECTED_ONLY, and with render=True above 16 (the
        overlay kernel draws all instances of an image in one pass).
        measure=True (keyword only): the dict gains "measurements", myolo.measure.properties of the image's instances in the order of class_ids:
        area, visible_area (the part no earlier instance covers), perimeter, euler_number (pieces minus holes), bbox, centroid, major / minor
        axis length, orientation, eccentricity and the raw records of 13 exact integer sums they come from -- measure.measure_dense of the
        full_masks planes integer for integer, in the frame mask_frame names.  The sums are taken on the device (Net.measure_masks, DESIGN.md
        section 25) whatever mask_format is; about 100 bytes per instance come down.  myolo.measure.table / write_csv write them out.  Not
        supported together with config.DETECT_MASKS_FOR_SELECTED_ONLY (ValueError)."""
        cfg = self.config
        D.check_args(cfg, [image], mask_frame, mask_format, render, max_detections, measure)
        assert self.mode == 'inference'
        if weights_dir is not None:
            self.load_weights(weights_dir)
        x, canvas = self._stager().stage_one(image, render)
        mask_d = feature = None
        if bool(getattr(cfg, "DETECT_MASKS_FOR_SELECTED_ONLY", False)):
            _, det_d, feature = self.net.predict_detections(x)             # the mask head runs in dense_masks, on the survivors only
        else:
            predict = self.net.predict_graphed if getattr(cfg, "INFERENCE_HIP_GRAPH", True) else self.net.predict
            _, det_d, mask_d = predict(x)                                  # device tensors
        selection = D.Selection.of_batch(self.net, det_d, 1, cs_threshold, cfg.IMAGE_SHAPE, max_detections)
        out = D.batch_results(self._stager(), det_d, mask_d, selection, self._frames([image], mask_frame), mask_format, canvas, feature,
                              measure=measure)
        return self._save_rendered(out, save_path) if render else out

    def detect_many(self, images, weights_dir=None, cs_threshold=0.35, in_flight=3, mask_frame="image", mask_format="dense", render=False, *,
                    max_detections=None, measure=False):
        """detect() for a sequence of images at the throughput of Net.predict_stream: the images go through the inference graph in batches of
        config.BATCH_SIZE with `in_flight` batches running at once (one stream / hipGraph / scratch per lane: the launch-bound trunk of one
        batch under the matrix-pipe-bound mask head of another), and every image gets detect()'s own selection and unmolding
        (model.py:1238-1328).  The images may have any sizes, mixed in one call: a batch whose images are all at config.IMAGE_SHAPE goes up as its
        bytes, any other batch is resized on the device (Net.resize_to_frame).  Returns one result dict per image, equal to
        detect(image, mask_frame=mask_frame)[0].
        mask_format="rle" (see detect; ValueError with config.DETECT_MASKS_FOR_SELECTED_ONLY): rle_masks in place of full_masks, and the
        post-processing runs once per BATCH -- the selection of all its images on the host from the one detection download, one [B, K] upload,
        one Net.rle_masks call whose two downloads are a few KB -- where the dense form pastes and downloads per image.
        mask_format="polygon" (see detect): polygons in place of full_masks, once per batch in the same way (one Net.contour_masks call).
        render=True (see detect; nothing is written to disk here): every dict gains "rendered", drawn once per BATCH on the bytes the batch went
        up as -- one Net.render_instances call, one download of the batch's overlays.  With mask_format="rle" no dense mask exists anywhere.
        max_detections=K (see detect): the selection of every batch runs on the device -- one launch, B * K * 7 words down -- and the batch's
        [B,R,6] detections are not downloaded.
        measure=True (see detect): every dict gains "measurements", taken once per BATCH -- one Net.measure_masks call over all the slots of
        its images, one download of 104 bytes per slot."""
        cfg = self.config
        images = list(images)
        D.check_args(cfg, images, mask_frame, mask_format, render, max_detections, measure)
        assert self.mode == 'inference'
        if weights_dir is not None:
            self.load_weights(weights_dir)
        B = int(cfg.BATCH_SIZE)
        groups = [images[lo:lo + B] for lo in range(0, len(images), B)]
        stager = self._stager()
        stager.reserve(in_flight, groups)
        canvases = {}                                    # batch -> its canvas, until it is drawn

        def batches():
            for bi, grp in enumerate(groups):
                x, canvases[bi] = stager.stage(bi, grp, render)
                yield x
        out = []
        for bi, (_, det_d, mask_d) in enumerate(self.net.predict_stream(batches(), in_flight=in_flight)):
            selection = D.Selection.of_batch(self.net, det_d, len(groups[bi]), cs_threshold, cfg.IMAGE_SHAPE, max_detections)
            out += D.batch_results(stager, det_d, mask_d, selection, self._frames(groups[bi], mask_frame), mask_format, canvases.pop(bi),
                                   measure=measure)
        return out

    def _save_rendered(self, results, save_path):
        """detect(render=True)'s file: save_path/InferMaskYOLO-<k>.png for result k of the call (the reference saves its figure under save_path
        too, model.py:1322-1328)"""
        if save_path is not None:
            from .render import write_png
            os.makedirs(save_path, exist_ok=True)
            for k, r in enumerate(results):
                write_png(os.path.join(save_path, "InferMaskYOLO-%d.png" % k), r["rendered"])
        return results

    def _select_and_unmold(self, det_img, mask_img, image_shape, cs_threshold, feature=None, det_host=None):
        """detect()'s dense post-processing of ONE image: det_img [R,6], mask_img [R,mh,mw,C] (None: the mask head runs on the survivors, over
        `feature`) device tensors, det_host = det_img's host copy if the caller has it.  -> its result dict."""
        det_h = det_img.cpu().numpy() if det_host is None else det_host
        selection = D.Selection(det_h[None], 1, cs_threshold, self.config.IMAGE_SHAPE)
        return D.batch_results(self._stager(), det_img.unsqueeze(0), None if mask_img is None else mask_img.unsqueeze(0), selection,
                               [image_shape], feature=feature)[0]

    # ------------------------------------------------------------------ evaluation
    def evaluate(self, dataset, cs_threshold=0.35, max_samples=None, in_flight=3, *, max_detections=None):
        """Mask and box average precision of detect()'s output on a dataset (myolo/evaluate.py) -> Evaluator.result().
        dataset: an object load_image_gt reads (as train() takes), or a sequence of (image, class_ids, boxes, masks) rows as load_image_gt
        returns them.  The images stream through the inference graph exactly as in detect_many and every image gets detect()'s own selection;
        the overlap of each selected detection's PASTED mask with each ground-truth mask is counted on the device (myolo_mask_overlap_counts:
        the paste of myolo_unmold_masks, pixel for pixel) -- K x T integers come down per image, no full-size mask is written or downloaded.
        An image's ground truth is its first MAX_GT_INSTANCES instances (what a training batch carries).
        max_detections=K (see detect): up to K detections per image are scored instead of ten, selected on the device."""
        cfg = self.config
        assert self.mode == 'inference'
        D.check_max_detections(cfg, max_detections)
        if hasattr(dataset, "load_segments"):          # (myolo.coco: the ground truth is decoded on the device, load_mask is never called)
            return self._evaluate_segments(dataset, cs_threshold, max_samples, in_flight, max_detections)
        if hasattr(dataset, "image_ids"):
            ids = list(dataset.image_ids)
            if max_samples is not None:
                ids = ids[:max_samples]
            info = [list(mutils.load_image_gt(dataset, cfg, i, use_mini_mask=cfg.USE_MINI_MASK)) for i in ids]
        else:
            info = list(dataset) if max_samples is None else list(dataset)[:max_samples]
        for row in info:
            assert list(row[0].shape) == list(cfg.IMAGE_SHAPE) and row[0].dtype == 'uint8'
        B, T = int(cfg.BATCH_SIZE), int(cfg.MAX_GT_INSTANCES)
        H, W = int(cfg.IMAGE_SHAPE[0]), int(cfg.IMAGE_SHAPE[1])
        stager = self._stager()
        slots = stager.reserve(in_flight)
        gt_ring = stager.pinned("gt", slots, (B, H, W, T))               # the ground truth rides beside the images, slot for slot
        truth = collections.deque()

        def batches():
            for bi, lo in enumerate(range(0, len(info), B)):
                grp = info[lo:lo + B]
                x, _ = stager.stage(bi, [r[0] for r in grp])
                gstage = gt_ring[bi % slots]
                gm = gstage.numpy()
                gm.fill(0)                                                   # (the planes of a short last batch's padding stay 0; ignored below)
                gt_ids, gt_boxes = np.zeros((B, T), np.int32), np.zeros((B, T, 4), np.int32)
                for k, (_, class_ids, boxes, masks) in enumerate(grp):
                    m = min(T, int(class_ids.shape[0]))                      # the first MAX_GT_INSTANCES, in order (BatchGenerator._encode's layout)
                    gt_ids[k, :m] = class_ids[:m]
                    gt_boxes[k, :m] = boxes[:m]
                    for j in range(m):
                        gm[k, :, :, j] = masks[:, :, j]
                truth.append((len(grp), gstage.to(self.net.dev, non_blocking=True), gt_ids, gt_boxes))
                yield x
        return self._evaluate_stream(batches(), truth, cs_threshold, in_flight, max_detections)

    def _evaluate_segments(self, dataset, cs_threshold, max_samples, in_flight, max_detections=None):
        """evaluate() on a dataset with load_segments (myolo.coco): per batch the image bytes, the segments of every image's
        first MAX_GT_INSTANCES annotations and the index tables go up, and myolo_segment_masks writes the ground-truth masks and their boxes on the
        device -- no mask is filled on the host, no [B,H,W,T] bytes cross PCIe.  A segment that sets no pixel of the network frame is found by its
        area (myolo_mask_overlap_counts' area_gt) and made padding in _evaluate_stream: it is dropped AFTER the cut to MAX_GT_INSTANCES, where
        load_image_gt drops it before (with at most MAX_GT_INSTANCES segments per image the two routes give equal results)."""
        cfg = self.config
        B, T = int(cfg.BATCH_SIZE), int(cfg.MAX_GT_INSTANCES)
        H, W = int(cfg.IMAGE_SHAPE[0]), int(cfg.IMAGE_SHAPE[1])
        info = self._collect_segments(dataset, max_samples, first=T)
        stager = self._stager()
        stager.reserve(in_flight)
        dev = self.net.dev
        truth = collections.deque()

        def batches():
            for bi, lo in enumerate(range(0, len(info), B)):
                grp = info[lo:lo + B]
                x, _ = stager.stage(bi, [r[0] for r in grp])
                gt_ids = np.zeros((B, T), np.int32)
                for k, r in enumerate(grp):
                    gt_ids[k, :r[1].shape[0]] = r[1]
                # (the slots of a short last batch's padding are empty)
                tables = [torch.from_numpy(a).to(dev) for a in mutils.segment_tables([(r[2], r[3], r[5]) for r in grp], B, T, H, W)]
                gt_masks = torch.empty((B, H, W, T), dtype=torch.uint8, device=dev)
                gt_boxes = torch.empty((B, T, 4), dtype=torch.int32, device=dev)
                self.net.segment_masks(tables, gt_masks, gt_boxes)
                truth.append((len(grp), gt_masks, gt_ids, gt_boxes, True))
                yield x
        return self._evaluate_stream(batches(), truth, cs_threshold, in_flight, max_detections)

    def evaluate_shapes_stream(self, n_images, seed=0, start_index=0, cs_threshold=0.35, in_flight=3, *, max_detections=None):
        """evaluate() on images start_index .. start_index + n_images - 1 of the synthetic Shapes stream with the inputs AND the ground truth
        produced on the device (myolo.shapes.ShapesProducer: bit-identical to ShapesDataset / load_image_gt): nothing but the detections' rows and
        the overlap counts crosses PCIe, so this runs at the speed of the inference forward.  max_detections: see evaluate."""
        from .shapes import ShapesProducer
        cfg = self.config
        assert self.mode == 'inference'
        D.check_max_detections(cfg, max_detections)
        B = int(cfg.BATCH_SIZE)
        prod = ShapesProducer(cfg, seed=seed, device=self._device)
        truth = collections.deque()

        def batches():
            for lo in range(0, n_images, B):
                d = prod.batch(list(range(start_index + lo, start_index + lo + B)))     # (a short last batch runs into the next images; ignored below)
                truth.append((min(B, n_images - lo), d["gt_masks"], d["gt_ids"], d["gt_boxes"]))
                yield d["images"]
        return self._evaluate_stream(batches(), truth, cs_threshold, in_flight, max_detections)

    def _evaluate_stream(self, batches, truth, cs_threshold, in_flight, max_detections=None):
        """the common part of evaluate() / evaluate_shapes_stream(): `batches` yields [B,H,W,3] device images and appends each batch's
        (images that count, gt_masks [B,H,W,T] device, gt_ids [B,T], gt_boxes [B,T,4] host or device) to the deque `truth`; a fifth element True
        (_evaluate_segments): a slot whose ground-truth plane is empty is padding whatever its class id."""
        from .evaluate import Evaluator
        ev = Evaluator()
        for _, det_d, mask_d in self.net.predict_stream(batches, in_flight=in_flight):
            entry = truth.popleft()
            n, gt_d, gt_ids, gt_boxes = entry[:4]
            drop_empty = len(entry) > 4
            selection = D.Selection.of_batch(self.net, det_d, n, cs_threshold, self.config.IMAGE_SHAPE, max_detections)
            inter, area_pred, area_gt, win = D.overlap_counts(self._stager(), det_d, mask_d, selection, gt_d)
            gt_ids, gt_boxes = [t.cpu().numpy() if torch.is_tensor(t) else t for t in (gt_ids, gt_boxes)]
            if drop_empty:
                gt_ids = np.where(area_gt[:gt_ids.shape[0]] > 0, gt_ids, 0)
            for k in range(n):
                _, class_ids, scores = selection.picked[k]
                m = len(scores)
                ev.add_image(scores, class_ids, gt_ids[k], inter[k, :m], area_pred[k, :m], area_gt[k], win[k, :m], gt_boxes[k])
        return ev.result()

    def _decode_masks_device(self, det, masks, image_shape):
        """decode_masks (model.py:1330-1391) with the unmold/paste of every detection on the GPU (detect.paste): det [N,6], masks [N,mh,mw,C]
        device tensors of one image.  The zero-area boxes are dropped here; detect()'s selection has dropped them before it pastes."""
        det_h = det.cpu().numpy()
        keep = np.where((det_h[:, 2] - det_h[:, 0]) * (det_h[:, 3] - det_h[:, 1]) > 0)[0]     # model.py:1373-1380
        if keep.shape[0] != det_h.shape[0]:
            idx = torch.as_tensor(keep, device=det.device)
            det, masks, det_h = det.index_select(0, idx), masks.index_select(0, idx), det_h[keep]
        full = D.paste(det, masks, image_shape) if len(keep) else np.empty((int(image_shape[0]), int(image_shape[1]), 0))
        return det_h[:, :4], det_h[:, 5].astype(np.int32), det_h[:, 4], full

    def decode_masks(self, detections, myolo_mask, image_shape):
        """model.py:1330-1391 (numpy in / numpy out; the unmolding runs on the GPU)."""
        assert len(detections) == 1
        assert len(myolo_mask) == 1
        assert list(image_shape) == list(self.config.IMAGE_SHAPE)
        if torch.cuda.is_available():
            dev = self.net.dev
            return self._decode_masks_device(torch.as_tensor(np.ascontiguousarray(detections[0], np.float32), device=dev),
                                             torch.as_tensor(np.ascontiguousarray(myolo_mask[0], np.float32), device=dev), image_shape)
        detection, masks_all = detections[0], myolo_mask[0]
        N = len(detection)
        boxes = detection[:N, :4]
        scores = detection[:N, 4]
        class_ids = detection[:N, 5].astype(np.int32)
        masks = masks_all[np.arange(N), :, :, class_ids]
        exclude_ix = np.where((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) <= 0)[0]
        if exclude_ix.shape[0] > 0:
            boxes = np.delete(boxes, exclude_ix, axis=0)
            class_ids = np.delete(class_ids, exclude_ix, axis=0)
            scores = np.delete(scores, exclude_ix, axis=0)
            masks = np.delete(masks, exclude_ix, axis=0)
            N = class_ids.shape[0]
        full_masks = [mutils.unmold_mask(masks[i], boxes[i], image_shape) for i in range(N)]
        full_masks = np.stack(full_masks, axis=-1) if full_masks else np.empty(tuple(image_shape[:2]) + (0,))
        return boxes, class_ids, scores, full_masks
