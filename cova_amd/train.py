"""BlobNet training for the front end this build runs behind (utils/train-blobnet.py, utils/data/*.py of the reference).

  read_tfrecords  TFRecord files as `tfrecordsink` / covahip_tfrecord_example write them -> frames + labels
  slide           utils/data/slide.py slide_dataset(skip=True): non-overlapping stacks of T = 4 frames, newest first
  init_weights    the Keras default initialisation of the reference model, as a flat weight array (cova_amd/weights.py order)
  TrainerSet      K models of one geometry in one trainer (covahip_train_*: forward, backward and Adam in HIP, one launch of each
                  kernel per step of all models) and the epoch loop
  Trainer         one model: a TrainerSet of one
  TrainData       frames and labels resident on the device (.append / .append_device from host / device memory, .gather /
                  .gather_device: the batch a sample array describes, to host / device memory)
  windows         the windows of a model's recordings as a table; epoch_samples: the table as one epoch's sample array, reordered,
                  mirrored, reversed; plain_samples: the table's windows as they are (validation, scoring); split_frames_tail;
                  balanced_samples: an epoch redrawn half from busy, half from quiet samples (TrainData.label_mass)
                  TrainerSet / Trainer .step_data, .evaluate_data, .fit_data take their batches from a TrainData by such arrays
  alignment       per recording, where the labels stand against the records: TrainData.align counts on the device, align_scores
                  and align_drift read the counts; windows / epoch_samples(label_shift=) apply the shift found

    python -m cova_amd.train RECORDS... -o blobnet.cvhw [--epochs 20 --batch 4 --seed 0 --h-mb 45 --w-mb 80]

writes a weight file that covahip_blobnet_load / BlobNetInfer / the blobnetfilter element load unchanged.

    python -m cova_amd.train --set -o OUTDIR CAM0.tfrecord CAM1.tfrecord CAM2a.tfrecord,CAM2b.tfrecord

trains one model per argument (several files of one model joined with commas; model k initialised and seeded with --seed + k)
and writes OUTDIR/CAM0.cvhw, OUTDIR/CAM1.cvhw, OUTDIR/CAM2a.cvhw: a model set for covahip_blobnet_load_set / BlobNetInfer([...]).
No TensorFlow or protobuf is needed: the record framing and the Example message are parsed here.

Held-out evaluation and resume (include/covahip.h, "Evaluation and resume"):

    python -m cova_amd.train RECORDS... -o blobnet.cvhw --val-frac 0.2 --keep best --checkpoint run.cvhs
    python -m cova_amd.train RECORDS... -o blobnet.cvhw --val-frac 0.2 --keep best --checkpoint run.cvhs --resume run.cvhs
    python -m cova_amd.train --eval-only blobnet.cvhw TODAY.tfrecord

--val FILES names validation records instead of splitting a tail off (with --set one comma-joined argument per model).  Every
epoch then reports the loss / precision / recall / IoU of the validation part in inference mode (moving BN statistics, no
dropout); --keep best writes the weights of the epoch with the lowest validation loss.  --checkpoint writes the whole trainer
state after every epoch and --resume continues from it, bit for bit where the interrupted run would have gone.  --eval-only
trains nothing: it prints one JSON line per model with the score of a weight file on the given records.

Fine-tuning (include/covahip.h, "Fine-tuning"): adapt a deployed model to the camera --eval-only showed to have drifted,

    python -m cova_amd.train NEWCAM.tfrecord -o adapted.cvhw --init blobnet.cvhw --freeze encoder --freeze-bn --epochs 5

--init starts from a weight file instead of a fresh initialisation (with --set: one file for every model, or a directory of
per-model files named as --set -o writes them).  --freeze takes layer groups (enc0..enc3, dec0..dec3, or encoder / decoder):
their weights are not trained and no gradient work is spent on them.  --freeze-bn keeps every BatchNorm layer on the moving
statistics of the base model instead of the statistics of a batch of 4.  --resume with the same flags continues exactly; the
plan is not part of the checkpoint.

The camera's post (include/covahip.h, "Training with a post"): train and score a model with the ignore region and the mask
threshold it is served with,

    python -m cova_amd.calibrate --weights blobnet.cvhw -o post.json --ignore-rects 0,0,320,48 HELDOUT.tfrecord
    python -m cova_amd.train NEWCAM.tfrecord -o adapted.cvhw --init blobnet.cvhw --post post.json
    python -m cova_amd.train --eval-only adapted.cvhw TODAY.tfrecord --post post.json

--post takes the sidecar calibrate wrote (with --set: one file for every model, or a directory of <stem>.json per model, named
as --set -o names weight files); --ignore-rects L,T,W,H[+L,T,W,H...] and --mask-threshold P give the same for a camera without
a sidecar.  Macroblocks in the ignore region take no part in the loss, its gradient or the metrics, and the metrics count
logit > threshold as serving does.  The post is not part of the checkpoint either: --resume takes it from the command line again.

Matrix-core arithmetic (include/covahip.h, "Training arithmetic"): --math matrix runs the convolutions of every step and
evaluation as fp32 implicit GEMMs on the matrix cores, two to five times faster per step; --math exact (the default) is the
trainer as it always was.  A run is bit-reproducible within its mode; the mode is not part of the checkpoint, and a checkpoint
of one mode resumes in the other.  It combines with every other flag.

Training from resident frames (include/covahip.h, "Training data"): every window of a recording, mirrored, reversed, reshuffled,

    python -m cova_amd.train CAM.tfrecord -o blobnet.cvhw --windows overlap --stride 1,2 --flip xy --reverse --shuffle --data-seed 1

Any of these six flags keeps the frames on the device as two-byte records (TrainData) and builds each step's batch there from a
table of frame indices (windows, epoch_samples; TrainerSet.fit_data / evaluate_data).  Every file is one segment that no window
crosses; --windows overlap takes all F - 3 windows of F frames instead of F / 4; --stride, --flip and --reverse are drawn per
sample and epoch and --shuffle reorders every epoch, all as pure functions of (--data-seed, epoch, model), so --resume with the
same flags continues exactly.  Validation windows are never augmented.  Without these flags the program runs as it always has.

Balanced epochs (utils/data/balance.py of the reference): most windows of a surveillance recording are empty road,

    python -m cova_amd.train CAM.tfrecord -o blobnet.cvhw --windows overlap --shuffle --balance 100

--balance N also trains from the resident data set.  A window is busy when the frame that labels it carries at least N labelled
macroblocks outside the camera's ignore region (counted on the device, TrainData.label_mass; the reference uses 100 at 45x80);
every epoch keeps its length and draws each sample from the busy or the quiet windows with probability 1/2, each half walked in
the epoch's order (balanced_samples).  The draws are a pure function of (--data-seed, epoch, model) too, and --resume takes
--balance from the command line again.  Validation windows are never balanced, and --eval-only refuses the flag.

Label alignment (include/covahip.h, covahip_train_data_align): records and labels come from different decoders, and a frame one
of them dropped moves every label against its record without any score showing it,

    python -m cova_amd.train CAM.tfrecord --windows overlap --align-report 8
    python -m cova_amd.train CAM.tfrecord -o blobnet.cvhw --windows overlap --label-shift auto

--align-report [S] trains nothing: per recording it counts on the device, for every frame shift s in -S .. S, the macroblocks
that move in the records of frame f AND are labelled in frame f + s (B) and those that do either (U), prints the table with the
best shift (largest B / U; TrainData.align, align_scores) and lists the frames where the best shift of a block of --align-window
frames changes (align_drift): a frame lost half-way.  --label-shift N labels every window by its labelling frame + N, the table
of windows shrunk so that this frame stays inside the recording (windows / epoch_samples label_shift); --label-shift auto[:S]
measures each recording's own N and stops, naming the recording, when there is none, when it sits at +-S, or when it changes
inside the recording.  Both need --windows.  The shift is a pure function of the data and the arguments: --resume stays exact.

    python -m cova_amd.train CAM.tfrecord --windows overlap --record-report [--save-inputs CAM.inputs.json]

--record-report trains nothing either: per recording it counts the records on the device (TrainData.record_stats, the input
monitor's quantities) and prints the class and vector marginals, the GoP estimate, the still share, the share of labelled
macroblocks whose record is all skip and the share of moving macroblocks that are labelled -- whether the records carry the labels
at all.  --save-inputs writes the counts of all recordings together: the baseline python -m cova_amd.monitor --input-baseline
compares a deployed camera with.
"""
from __future__ import annotations

import argparse
import ctypes as C
import functools
import json
import math
import os
import struct
import sys

import numpy as np

from . import _lib as L
from . import weights as W

FEATURES = ("mb_type", "mv_x", "mv_y", "gt")

# ------------------------------------------------------------------------------------------------ TFRecord reader
_CRC_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0x82F63B78 if _c & 1 else _c >> 1
    _CRC_TABLE.append(_c)


_CRC_NP = np.array(_CRC_TABLE, dtype=np.uint32)


def _crc_raw_bytes(c: int, data) -> int:
    """The CRC register after `data`, one byte at a time from register c (no pre / post inversion)."""
    tab = _CRC_TABLE
    for b in data:
        c = tab[(c ^ b) & 0xFF] ^ (c >> 8)
    return c


@functools.lru_cache(maxsize=16)
def _shift_tables(n: int) -> np.ndarray:
    """[4][256] tables of the linear map 'register after n zero bytes': shift(r) = xor of T[k][(r >> 8k) & 255]."""
    basis = np.array([1 << i for i in range(32)], dtype=np.uint32)
    r = basis.copy()
    for _ in range(n):
        r = _CRC_NP[r & 0xFF] ^ (r >> np.uint32(8))
    tabs = np.zeros((4, 256), dtype=np.uint32)
    v = np.arange(256, dtype=np.uint32)
    for k in range(4):
        for bit in range(8):
            tabs[k] ^= np.where((v >> np.uint32(bit)) & np.uint32(1), r[8 * k + bit], np.uint32(0))
    return tabs


def crc32c(data: bytes) -> int:
    """CRC-32C (Castagnoli, reflected), as TFRecord frames use it.

    Long inputs are cut into n equal chunks whose registers (from 0) are computed side by side in numpy; the register is
    linear over GF(2), so the chunks fold in order as r = shift_L(r) ^ chunk_k, with shift_L the map of L zero bytes.
    About 30 MB/s on a one-frame 45x80 record, 60 MB/s on an eight-frame one, 150 MB/s on 1 MB (a byte loop: 10 MB/s)."""
    data = memoryview(data).cast("B")
    size = len(data)
    if size < 2048:
        return _crc_raw_bytes(0xFFFFFFFF, data) ^ 0xFFFFFFFF
    L = 1 << max(5, (int(math.isqrt(size)) // 2).bit_length() - 1)   # chunk length: a power of two near sqrt(size) / 2
    n = size // L
    chunks = np.frombuffer(data[:n * L], dtype=np.uint8).reshape(n, L)
    r = np.zeros(n, dtype=np.uint32)
    for j in range(L):
        r = _CRC_NP[(r ^ chunks[:, j]) & 0xFF] ^ (r >> np.uint32(8))
    t0, t1, t2, t3 = (list(map(int, t)) for t in _shift_tables(L))
    c = 0xFFFFFFFF
    for ck in r.tolist():
        c = t0[c & 0xFF] ^ t1[(c >> 8) & 0xFF] ^ t2[(c >> 16) & 0xFF] ^ t3[c >> 24] ^ ck
    return _crc_raw_bytes(c, data[n * L:]) ^ 0xFFFFFFFF


def masked_crc32c(data: bytes) -> int:
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def _varint(buf: bytes, pos: int):
    v = shift = 0
    while True:
        if pos >= len(buf):
            raise ValueError("truncated varint")
        b = buf[pos]
        pos += 1
        v |= (b & 0x7F) << shift
        if not b & 0x80:
            return v, pos
        shift += 7
        if shift > 63:
            raise ValueError("varint too long")


def _fields(buf: bytes):
    """(field number, payload) of the length-delimited fields of a protobuf message; other wire types are skipped."""
    pos = 0
    while pos < len(buf):
        key, pos = _varint(buf, pos)
        field, wt = key >> 3, key & 7
        if wt == 2:
            n, pos = _varint(buf, pos)
            if pos + n > len(buf):
                raise ValueError("truncated field")
            yield field, buf[pos:pos + n]
            pos += n
        elif wt == 0:
            _, pos = _varint(buf, pos)
        elif wt == 1:
            pos += 8
        elif wt == 5:
            pos += 4
        else:
            raise ValueError(f"unsupported wire type {wt}")
    if pos != len(buf):
        raise ValueError("truncated message")


def parse_example(payload: bytes) -> dict:
    """tf.train.Example -> {feature name: [bytes, ...]} for its bytes_list features."""
    out = {}
    for f, features in _fields(payload):               # Example.features
        if f != 1:
            continue
        for g, entry in _fields(features):             # Features.feature (map entry)
            if g != 1:
                continue
            key, value = None, b""
            for h, v in _fields(entry):
                if h == 1:
                    key = v.decode()
                elif h == 2:
                    value = v
            strings = []
            for k, blist in _fields(value):            # Feature.bytes_list
                if k == 1:
                    strings += [s for m, s in _fields(blist) if m == 1]   # BytesList.value
            out[key] = strings
    return out


def iter_records(data: bytes):
    """Payloads of a TFRecord file: u64 length, masked CRC of the length, payload, masked CRC of the payload."""
    pos = 0
    while pos < len(data):
        if pos + 12 > len(data):
            raise ValueError(f"truncated record header at byte {pos}")
        (n,) = struct.unpack_from("<Q", data, pos)
        (c1,) = struct.unpack_from("<I", data, pos + 8)
        if masked_crc32c(data[pos:pos + 8]) != c1:
            raise ValueError(f"length CRC mismatch at byte {pos}")
        if pos + 12 + n + 4 > len(data):
            raise ValueError(f"truncated record at byte {pos}")
        payload = data[pos + 12:pos + 12 + n]
        (c2,) = struct.unpack_from("<I", data, pos + 12 + n)
        if masked_crc32c(payload) != c2:
            raise ValueError(f"payload CRC mismatch at byte {pos}")
        yield payload
        pos += 12 + n + 4


def read_tfrecords(paths, h_mb: int, w_mb: int):
    """frames u8 [F][h][w][4] (bytes 0..2 = mb_type / mv_x / mv_y, byte 3 = 0) and gt u8 [F][h][w] of every string of
    every record, in file and record order -- one frame per record or several (the sink's `gop` form, zero-filled strings
    included, as utils/data/parse.py decodes them).  A CRC mismatch, a truncated record or a string of the wrong size raises."""
    if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__"):
        paths = [paths]
    hw = h_mb * w_mb
    frames, gts = [], []
    for path in paths:
        with open(path, "rb") as f:
            data = f.read()
        for payload in iter_records(data):
            ex = parse_example(payload)
            missing = [k for k in FEATURES if k not in ex]
            if missing:
                raise ValueError(f"{path}: record lacks features {missing}")
            n = len(ex["mb_type"])
            if any(len(ex[k]) != n for k in FEATURES):
                raise ValueError(f"{path}: features of different lengths")
            for k in FEATURES:
                for s in ex[k]:
                    if len(s) != hw:
                        raise ValueError(f"{path}: {k} string of {len(s)} bytes, expected {h_mb}x{w_mb}")
            for i in range(n):
                fr = np.zeros((h_mb, w_mb, 4), np.uint8)
                for ch in range(3):
                    fr[..., ch] = np.frombuffer(ex[FEATURES[ch]][i], np.uint8).reshape(h_mb, w_mb)
                frames.append(fr)
                gts.append(np.frombuffer(ex["gt"][i], np.uint8).reshape(h_mb, w_mb))
    if not frames:
        return np.zeros((0, h_mb, w_mb, 4), np.uint8), np.zeros((0, h_mb, w_mb), np.uint8)
    return np.stack(frames), np.stack(gts)


def slide(frames: np.ndarray, gt: np.ndarray, t: int = W.T):
    """slide_dataset(skip=True): frames [4k..4k+3] -> one stack [4k+3, 4k+2, 4k+1, 4k] (row block i = frame newest - i, the
    metapreprocess layout [t*h][w][4]) labelled with frame 4k+3's gt.  A trailing incomplete group is dropped."""
    n = frames.shape[0] // t
    f, h, w, _ = frames.shape
    g = frames[:n * t].reshape(n, t, h, w, 4)[:, ::-1]
    stacks = np.ascontiguousarray(g.reshape(n, t * h, w, 4))
    labels = np.ascontiguousarray(gt[t - 1:n * t:t])
    return stacks, labels


# ------------------------------------------------------------------------------------------------ initialisation
def _truncated_normal(rng, std, shape):
    """Normal(0, std) resampled until inside 2 std (tf.random.truncated_normal)."""
    out = rng.normal(0.0, std, shape)
    bad = np.abs(out) > 2 * std
    while bad.any():
        out[bad] = rng.normal(0.0, std, int(bad.sum()))
        bad = np.abs(out) > 2 * std
    return out


def he_normal(rng, fan_in, shape):
    """Keras VarianceScaling(2, fan_in, truncated_normal): std sqrt(2 / fan_in) after the truncation at 2 sigma."""
    return _truncated_normal(rng, math.sqrt(2.0 / fan_in) / 0.87962566103423978, shape)


def glorot_uniform(rng, fan_in, fan_out, shape):
    lim = math.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, shape)


def init_weights(seed: int = 0) -> np.ndarray:
    """Keras-default initialisation of the reference model: he_normal conv / convT kernels (Keras fan_in: 9 * Cin for the
    Conv3D kernel [1,3,3,Cin,Cout], 16 * Cout for the Conv3DTranspose kernel [1,4,4,Cout,Cin]), glorot_uniform Conv1D
    kernels (fan 4 / 4) and final 1x1 kernel (fan 16 / 1), zero biases, BN gamma 1 / beta 0 / mean 0 / var 1."""
    rng = np.random.default_rng(seed)
    t = {}
    for name, shape in W.tensor_specs().items():
        kind = name.split(".", 1)[1]
        if kind == "conv.kernel":
            t[name] = he_normal(rng, shape[0] * shape[1] * shape[2], shape)
        elif kind == "up.kernel":
            t[name] = he_normal(rng, shape[0] * shape[1] * shape[2], shape)
        elif kind in ("tmix.w1", "tmix.w2"):
            t[name] = glorot_uniform(rng, W.T, W.T, shape)
        elif name == "final.kernel":
            t[name] = glorot_uniform(rng, 16, 1, shape)
        elif kind in ("bn.gamma", "bn.var"):
            t[name] = np.ones(shape)
        else:                                   # biases, beta, mean
            t[name] = np.zeros(shape)
    return W.flatten(t)


# ------------------------------------------------------------------------------------------------ host logic of the step
def keras_lr(epoch: int, base: float = 1e-3) -> float:
    """The reference's LearningRateScheduler: lr constant for epochs 0..9, times e^-0.1 at each later epoch."""
    return base * math.exp(-0.1 * max(0, epoch - 9))


def adam_lr_t(lr: float, step: int, beta1: float = 0.9, beta2: float = 0.999) -> float:
    """Keras Adam's step size at step t = step + 1: lr * sqrt(1 - b2^t) / (1 - b1^t)."""
    t = step + 1
    return lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)


def trainable_mask() -> np.ndarray:
    """True for every trained weight; False for the BN moving statistics."""
    parts = []
    for name, shape in W.tensor_specs().items():
        parts.append(np.full(int(np.prod(shape)), not name.endswith((".bn.mean", ".bn.var"))))
    return np.concatenate(parts)


# ------------------------------------------------------------------------------------------------ training plan (fine-tuning)
GROUPS = ("enc0", "enc1", "enc2", "enc3", "dec0", "dec1", "dec2", "dec3")   # bit order of covahip_train_plan.frozen_groups
BN_LAYERS = GROUPS[:7]                                                       # ... and of .bn_inference (dec3 has no BN)
_SHORTHANDS = {"encoder": GROUPS[:4], "decoder": GROUPS[4:]}


def _plan_names(arg, valid, what):
    if arg is None:
        return []
    if isinstance(arg, str):
        arg = [n for n in arg.split(",") if n]
    out = []
    for name in arg:
        if name == "all" and what == "bn_inference":
            out += valid
        elif name in _SHORTHANDS:
            out += [n for n in _SHORTHANDS[name] if n in valid]
        elif name in valid:
            out.append(name)
        else:
            raise ValueError(f"{what}: unknown name {name!r} (one of {', '.join(valid)}, encoder, decoder"
                             + (", all)" if what == "bn_inference" else ")"))
    return out


def plan_bits(freeze=(), bn_inference=()):
    """(frozen_groups, bn_inference) of a covahip_train_plan from names: "enc0".."enc3", "dec0".."dec3" (bn_inference: up to
    "dec2"), the shorthands "encoder" / "decoder", and bn_inference="all"; a comma-separated string or an iterable.  The
    bn_inference bits are the ones given: the library adds the frozen groups' layers.  Unknown names and a plan that freezes
    all eight groups (nothing left to train) are a ValueError."""
    fz = sum({1 << GROUPS.index(n) for n in _plan_names(freeze, GROUPS, "freeze")})
    bn = sum({1 << BN_LAYERS.index(n) for n in _plan_names(bn_inference, BN_LAYERS, "bn_inference")})
    if fz == 0xFF:
        raise ValueError("freeze: all eight groups frozen, nothing left to train")
    return fz, bn


def plan_names(frozen_groups: int, bn_inference: int) -> dict:
    """{"freeze": names, "bn_inference": names} of plan bits, in bit order."""
    return {"freeze": tuple(n for k, n in enumerate(GROUPS) if frozen_groups >> k & 1),
            "bn_inference": tuple(n for k, n in enumerate(BN_LAYERS) if bn_inference >> k & 1)}


# ------------------------------------------------------------------------------------------------ validation split, state blob
def split_tail(stacks: np.ndarray, labels: np.ndarray, frac: float):
    """((train stacks, train labels), (validation stacks, validation labels)): the LAST ceil(frac * N) samples validate, the
    rest trains.  A tail, not a shuffle: consecutive stacks of a camera are near-duplicates and a random split would leak.
    A frac that leaves either part empty is a ValueError."""
    n = int(stacks.shape[0])
    if labels.shape[0] != n:
        raise ValueError(f"{n} stacks but {labels.shape[0]} labels")
    n_val = int(math.ceil(frac * n - 1e-9))
    if not 0 < n_val < n:
        raise ValueError(f"validation fraction {frac} of {n} samples leaves {n_val} to validate and {n - n_val} to train")
    return (stacks[:n - n_val], labels[:n - n_val]), (stacks[n - n_val:], labels[n - n_val:])


STATE_MAGIC = 0x53485643      # "CVHS"
STATE_VERSION = 1
STATE_HEADER = struct.Struct("<IIIIii8fQ")
assert STATE_HEADER.size == 64


def read_state_header(data: bytes) -> dict:
    """The header, step counters and seeds of a trainer state blob (covahip_train_save_state), checked as the library checks
    it on load.  Raises ValueError naming what is wrong: truncated, bad magic, unsupported version, size mismatch or CRC mismatch."""
    if len(data) < 68:
        raise ValueError(f"truncated state blob: {len(data)} bytes, a header and a checksum take 68")
    magic, version, n_models, n_params, h_mb, w_mb, *scalars, user_tag = STATE_HEADER.unpack_from(data, 0)
    if magic != STATE_MAGIC:
        raise ValueError(f"bad magic {magic:#010x}: not a trainer state blob")
    if version != STATE_VERSION:
        raise ValueError(f"unsupported version {version} of the trainer state blob (this build reads {STATE_VERSION})")
    per_model = 16 + 3 * 4 * n_params
    want = 64 + n_models * per_model + 4
    if len(data) != want:
        kind = "truncated state blob" if len(data) < want else "size mismatch"
        raise ValueError(f"{kind}: {len(data)} bytes, {n_models} models of {n_params} parameters take {want}")
    (crc,) = struct.unpack_from("<I", data, want - 4)
    if crc32c(memoryview(data)[:want - 4]) != crc:
        raise ValueError("CRC mismatch: the state blob is corrupted")
    out = {"version": version, "n_models": n_models, "n_params": n_params, "h_mb": h_mb, "w_mb": w_mb, "user_tag": user_tag}
    out.update(zip(("lr", "beta1", "beta2", "eps", "bn_momentum", "bn_eps", "dropout", "smooth"), scalars))
    steps_seeds = [struct.unpack_from("<QQ", data, 64 + k * per_model) for k in range(n_models)]
    out["steps"] = [int(a) for a, _ in steps_seeds]
    out["seeds"] = [int(b) for _, b in steps_seeds]
    return out


def _eval_dict(res) -> dict:
    """loss and the micro-averaged precision / recall / IoU of a covahip_train_eval_result (0-denominators as fit treats them)."""
    tp, fp, fn = int(res.tp), int(res.fp), int(res.fn)
    return {"loss": float(res.loss), "precision": tp / max(1, tp + fp), "recall": tp / max(1, tp + fn),
            "iou": tp / max(1, tp + fp + fn), "samples": int(res.samples)}


def _val_fields(ev: dict) -> dict:
    return {"val_" + k: ev[k] for k in ("loss", "precision", "recall", "iou")}


def _check_fit_args(val, keep):
    if keep not in ("last", "best"):
        raise ValueError(f"keep = {keep!r}: 'last' or 'best'")
    if keep == "best" and val is None:
        raise ValueError("keep='best' needs validation data (val=...): the best epoch is the one with the lowest val_loss")


def _replace_file(path, data: bytes):
    tmp = str(path) + ".tmp"
    with open(tmp, "wb") as f:
        f.write(data)
    os.replace(tmp, path)


WEIGHT_FILE_BYTES = 64 + 4 * W.N_PARAMS
_BEST_HEAD = struct.Struct("<4sI")


MATH_MODES = ("exact", "matrix")    # COVAHIP_TRAIN_MATH_EXACT, COVAHIP_TRAIN_MATH_MATRIX


class _State:
    """Trainer state and best-epoch bookkeeping of TrainerSet and Trainer (both hold .handle, .ctx, ._lib)."""

    def state_bytes(self, epoch: int = 0) -> bytes:
        """The whole trainer as one blob (weights, moving statistics, Adam moments, step counters, dropout seeds of every model);
        `epoch` travels as the blob's user_tag."""
        n = C.c_size_t()
        L.check(self._lib.covahip_train_state_size(self.handle, C.byref(n)), "covahip_train_state_size")
        buf = np.zeros(n.value, np.uint8)
        L.check(self._lib.covahip_train_save_state(self.handle, epoch, buf.ctypes.data, n.value, C.byref(n)),
                "covahip_train_save_state", self.ctx.handle)
        return buf.tobytes()

    def load_state_bytes(self, data: bytes) -> int:
        """Continues where the trainer that saved `data` stood, bit for bit; returns the stored epoch.  A blob the library refuses
        raises CovahipError and leaves this trainer as it was."""
        tag = C.c_uint64()
        L.check(self._lib.covahip_train_load_state(self.handle, data, len(data), C.byref(tag)), "covahip_train_load_state",
                self.ctx.handle)
        self._set_step_counts(read_state_header(data)["steps"])
        return int(tag.value)

    def save_state(self, path, epoch: int = 0) -> None:
        _replace_file(path, self.state_bytes(epoch))

    def set_plan(self, freeze=(), bn_inference=()) -> None:
        """The training plan from the next step on (for every model of a set): `freeze` names layer groups that are not trained,
        `bn_inference` BatchNorm layers that normalise with their moving statistics and leave them alone (plan_bits for the
        names; a frozen group's BatchNorm is in inference mode anyway).  set_plan() restores full training.  The plan is not
        part of the trainer state: set it again after creating the trainer a state is loaded into."""
        fz, bn = plan_bits(freeze, bn_inference)
        L.check(self._lib.covahip_train_set_plan(self.handle, C.byref(L.TrainPlan(fz, bn))), "covahip_train_set_plan", self.ctx.handle)

    @property
    def plan(self) -> dict:
        """The effective plan as names: {"freeze": (...), "bn_inference": (...)}, the latter with the frozen groups' layers."""
        p = L.TrainPlan()
        L.check(self._lib.covahip_train_get_plan(self.handle, C.byref(p)), "covahip_train_get_plan")
        return plan_names(p.frozen_groups, p.bn_inference)

    def set_math(self, math: str) -> None:
        """The arithmetic of the convolutions from the next step or evaluation on (for every model of a set): "exact", the plain
        kernels (the default), or "matrix", the matrix-core implicit GEMMs (covahip_train_set_math).  Both are fp32 throughout;
        a run is bit-reproducible within its mode, not across the two.  Like the plan the mode is not part of the trainer
        state: a state saved in one mode loads in the other."""
        if math not in MATH_MODES:
            raise ValueError(f"math must be one of {', '.join(MATH_MODES)}, not {math!r}")
        L.check(self._lib.covahip_train_set_math(self.handle, MATH_MODES.index(math)), "covahip_train_set_math", self.ctx.handle)

    @property
    def math(self) -> str:
        m = C.c_int()
        L.check(self._lib.covahip_train_get_math(self.handle, C.byref(m)), "covahip_train_get_math")
        return MATH_MODES[m.value]

    def load_state(self, path) -> int:
        with open(path, "rb") as f:
            return self.load_state_bytes(f.read())

    # best epochs of fit(keep="best"): per model (val_loss, weight file bytes) or None
    def _best_update(self, k: int, loss: float, weights_bytes) -> None:
        if self._best[k] is None or loss < self._best[k][0]:      # ties: the earliest epoch stays
            self._best[k] = (loss, weights_bytes())

    def _best_save(self, checkpoint) -> None:
        """Next to a checkpoint: CHECKPOINT.best, so that a resumed run knows the best epoch before the interruption."""
        if any(b is None for b in self._best):
            return
        parts = [_BEST_HEAD.pack(b"CVHB", len(self._best))]
        for loss, data in self._best:
            parts += [struct.pack("<d", loss), data]
        _replace_file(str(checkpoint) + ".best", b"".join(parts))

    def _best_start(self, n_models: int, keep: str, checkpoint, start_epoch: int) -> None:
        self._best = [None] * n_models
        path = None if checkpoint is None else str(checkpoint) + ".best"
        if keep != "best" or not start_epoch or path is None or not os.path.exists(path):
            return
        with open(path, "rb") as f:
            data = f.read()
        per = 8 + WEIGHT_FILE_BYTES
        if len(data) != _BEST_HEAD.size + n_models * per or _BEST_HEAD.unpack_from(data)[:2] != (b"CVHB", n_models):
            raise ValueError(f"{path}: not the best-epoch file of a {n_models}-model training")
        for k in range(n_models):
            o = _BEST_HEAD.size + k * per
            self._best[k] = (struct.unpack_from("<d", data, o)[0], data[o + 8:o + per])


def _eval_out(res, sl, lg) -> dict:
    out = _eval_dict(res)
    if sl is not None:
        out["sample_loss"] = sl
    if lg is not None:
        out["logits"] = lg
    return out


def _epoch_text(ep: int, epochs: int, rec: dict, model=None) -> str:
    """The log line of an epoch record; `model` tags the line of a set's model."""
    val = "" if "val_loss" not in rec else (f" val_loss {rec['val_loss']:.4f} val_precision {rec['val_precision']:.4f} "
                                            f"val_recall {rec['val_recall']:.4f} val_iou {rec['val_iou']:.4f}")
    return (f"epoch {ep + 1}/{epochs}{'' if model is None else f' model {model}'}: loss {rec['loss']:.4f} "
            f"precision {rec['precision']:.4f} recall {rec['recall']:.4f}{val} lr {rec['lr']:.3g}")


# ------------------------------------------------------------------------------------------------ resident training data
SAMPLE = L.TRAIN_SAMPLE_DTYPE
_M64 = (1 << 64) - 1


def splitmix64(z):
    """The header's splitmix64 (include/covahip.h, "BlobNet training") on a u64 array, all arithmetic mod 2^64."""
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64)) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _segments(segments) -> list:
    out = [(int(a), int(b)) for a, b in segments]
    if any(a < 0 or b < a for a, b in out):
        raise ValueError(f"a segment is a half-open range of frame indices [a, b), got {out}")
    return out


def _strides(strides) -> tuple:
    strides = tuple(int(s) for s in ((strides,) if np.isscalar(strides) else strides))
    if not strides or min(strides) < 1:
        raise ValueError(f"strides = {strides}: at least one, each at least 1")
    return strides


def windows(segments, mode: str = "skip", strides=(1,), label_shift: int = 0) -> np.ndarray:
    """The windows of a model's segments (half-open ranges of frame indices of a TrainData, one contiguous recording each) as a
    table i64 [N][2] of (segment start, newest frame k) in canonical order: segment by segment, k ascending.  mode "skip": slide's
    groups, frames 4j .. 4j + 3 of the segment (k = start + 4j + 3); "overlap": every k of the segment.  Either way only k with
    k - 3 * min(strides) >= start: a window never crosses a segment boundary, and every window of the table fits at least one of
    the strides (epoch_samples picks among those that fit).
    label_shift = s (alignment): the label that belongs to record frame f stands at frame f + s, and epoch_samples(label_shift=s)
    labels a window by its labelling frame + s.  The table keeps that frame inside the segment for forward and reversed windows
    alike: s > 0 drops the k with k + s >= segment end; s < 0 writes start + |s| as the start, which the rule above then holds
    the oldest frame to.  0 is the table as it always was."""
    if mode not in ("skip", "overlap"):
        raise ValueError(f"mode = {mode!r}: 'skip' or 'overlap'")
    reach = (W.T - 1) * min(_strides(strides))
    s = int(label_shift)
    rows = []
    for a, b in _segments(segments):
        k = np.arange(a + W.T - 1, a + (b - a) // W.T * W.T, W.T) if mode == "skip" else np.arange(a, b)
        lo = a + max(-s, 0)
        k = k[(k - reach >= lo) & (k + max(s, 0) < b)].astype(np.int64)
        rows.append(np.stack([np.full(k.size, lo, np.int64), k], axis=1))
    return np.concatenate(rows) if rows else np.zeros((0, 2), np.int64)


def _draws(data_seed: int, epoch: int, model: int, site: int, n: int) -> np.ndarray:
    """r(site, i) for i in [0, n) of epoch_samples' docstring, u64 [n]."""
    word = ((int(epoch) << 20) | (int(model) << 4)) & _M64
    key = splitmix64(np.uint64(int(data_seed) & _M64) ^ splitmix64(np.uint64(word | site)))
    return splitmix64(key + np.arange(n, dtype=np.uint64))


def epoch_samples(table, strides=(1,), data_seed: int = 0, epoch: int = 0, model: int = 0, shuffle: bool = False, flip=(),
                  reverse: bool = False, label_shift=0) -> np.ndarray:
    """The covahip_train_sample array (dtype SAMPLE) of one epoch of one model over a windows() table: a pure function of its
    arguments, built on the header's splitmix64 (numpy's generators are not pinned across versions, and resume must be exact).
        key(site) = splitmix64(data_seed ^ splitmix64(epoch << 20 | model << 4 | site))
        r(site, i) = splitmix64(key(site) + i),   i = the window's canonical index (its row of the table)
    order: a stable argsort of r(0, i) when `shuffle`, else canonical; mirror x: r(1, i) >> 63 when "x" is in `flip`; mirror y:
    r(2, i) >> 63 when "y" is in it; time reversal: r(3, i) >> 63 when `reverse` -- the frames are then listed oldest first and
    the OLDEST frame labels the sample; stride: the (r(4, i) mod m)-th, in the order given, of the m strides s with
    k - 3 s >= segment start.  A forward window at stride s is frames (k, k - s, k - 2s, k - 3s) labelled by frame k.
    label_shift = s, or one s per row of the table (alignment; the table comes from windows(label_shift=s)): the sample is
    labelled by its labelling frame + s, forward or reversed.  Nothing else changes, no draw among them.
    The key's word keeps its three fields apart for 0 <= site < 16, 0 <= model < 2^16 and 0 <= epoch < 2^44; anything outside is
    a ValueError."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, 2)
    strides = _strides(strides)
    if not (0 <= int(model) < 1 << 16 and 0 <= int(epoch) < 1 << 44):
        raise ValueError(f"model = {model}, epoch = {epoch}: 0 <= model < 2^16 and 0 <= epoch < 2^44")
    if any(c not in ("x", "y") for c in flip):
        raise ValueError(f"flip = {flip!r}: 'x', 'y', both or neither")
    n = table.shape[0]

    def r(site):
        return _draws(data_seed, epoch, model, site, n)

    start, k = table[:, 0], table[:, 1]
    fits = np.stack([k - (W.T - 1) * s >= start for s in strides], axis=1) if n else np.zeros((0, len(strides)), bool)
    m = fits.sum(axis=1)
    if (m == 0).any():
        raise ValueError(f"none of the strides {strides} fits window {table[int(np.argmin(m))].tolist()} in its segment")
    pick = (r(4) % m.astype(np.uint64)).astype(np.int64)
    which = np.argmax(fits & (np.cumsum(fits, axis=1) - 1 == pick[:, None]), axis=1) if n else np.zeros(0, np.int64)
    step = np.asarray(strides, dtype=np.int64)[which]
    out = np.zeros(n, SAMPLE)
    frames = k[:, None] - step[:, None] * np.arange(W.T, dtype=np.int64)[None, :]      # newest first
    if reverse:
        rev = (r(3) >> np.uint64(63)).astype(bool)
        frames = np.where(rev[:, None], frames[:, ::-1], frames)
    out["frame"] = frames
    out["label"] = frames[:, 0] + np.broadcast_to(np.asarray(label_shift, dtype=np.int64), (n,))
    if "x" in flip:
        out["flags"] |= (r(1) >> np.uint64(63)).astype(np.uint32)
    if "y" in flip:
        out["flags"] |= (r(2) >> np.uint64(63)).astype(np.uint32) << np.uint32(1)
    if shuffle:
        out = out[np.argsort(r(0), kind="stable")]
    return np.ascontiguousarray(out)


def plain_samples(table, stride: int = 1) -> np.ndarray:
    """The table's windows as they are: canonical order, forward, unmirrored, at `stride` (validation and scoring)."""
    return epoch_samples(table, (stride,))


def balanced_samples(samples, mass, threshold: int, *, mass_first: int = 0, data_seed: int = 0, epoch: int = 0,
                     model: int = 0) -> np.ndarray:
    """An epoch's SAMPLE array redrawn so that busy and quiet samples come up with probability 1/2 each (the reference's
    utils/data/balance.py, threshold 100 at 45x80): as many samples as given, a pure function of its arguments.
    mass[i] = the label mass of frame mass_first + i (TrainData.label_mass).  A sample is busy when the mass of the frame that
    LABELS it -- the oldest frame of a reversed window -- is at least `threshold`.  B = the busy samples and Q = the quiet ones,
    each in the order given; either one empty is a ValueError (the reference would run an empty epoch).  With epoch_samples' key
    at site 5 and i the DRAW POSITION, c[j] = r(5, j) >> 63; nb[j] = the busy draws before j and nq[j] = j - nb[j]:
        out[j] = B[nb[j] mod len(B)] if c[j] else Q[nq[j] mod len(Q)]
    so each half is walked in order and wraps, as the reference's .repeat() does.  A sample drawn twice in an epoch carries the
    same stride, mirrors and direction both times: epoch_samples keys those draws by the window's canonical index, not by where
    the sample stands in the epoch."""
    samples = _samples(samples)
    mass = np.asarray(mass).reshape(-1)
    if not (0 <= int(model) < 1 << 16 and 0 <= int(epoch) < 1 << 44):
        raise ValueError(f"model = {model}, epoch = {epoch}: 0 <= model < 2^16 and 0 <= epoch < 2^44")
    at = samples["label"].astype(np.int64) - int(mass_first)
    if at.size and (at.min() < 0 or at.max() >= mass.size):
        raise ValueError(f"mass covers frames [{mass_first}, {int(mass_first) + mass.size}), the samples are labelled by frames "
                         f"{int(at.min()) + int(mass_first)} .. {int(at.max()) + int(mass_first)}")
    busy = mass[at] >= threshold
    b, q = np.flatnonzero(busy), np.flatnonzero(~busy)
    if not b.size or not q.size:
        raise ValueError(f"balance: {b.size} busy and {q.size} quiet samples at threshold {threshold}: both halves need at least one")
    n = samples.shape[0]
    c = (_draws(data_seed, epoch, model, 5, n) >> np.uint64(63)).astype(np.int64)
    nb = np.cumsum(c) - c
    nq = np.arange(n, dtype=np.int64) - nb
    return np.ascontiguousarray(samples[np.where(c != 0, b[nb % b.size], q[nq % q.size])])


def split_frames_tail(segments, frac: float):
    """(training segments, validation segments) of one model: the LAST ceil(frac * F) of its F frames validate.  The cut splits
    a segment in two, so no window straddles it (split_tail's rule, in frames).  A frac that leaves either part empty is a
    ValueError."""
    segments = _segments(segments)
    total = sum(b - a for a, b in segments)
    n_val = int(math.ceil(frac * total - 1e-9))
    if not 0 < n_val < total:
        raise ValueError(f"validation fraction {frac} of {total} frames leaves {n_val} to validate and {total - n_val} to train")
    train, val, left = [], [], total - n_val
    for a, b in segments:
        cut = min(b, a + left)
        left -= cut - a
        if cut > a:
            train.append((a, cut))
        if b > cut:
            val.append((cut, b))
    return train, val


class TrainData:
    """A device-resident training data set (include/covahip.h, "Training data"): frames as two-byte records with their label
    bytes, 3 bytes per macroblock.  The trainers take their batches from it by tables of frame indices (epoch_samples)."""

    def __init__(self, ctx, h_mb: int, w_mb: int, capacity: int):
        self.ctx, self.h, self.w, self.capacity = ctx, h_mb, w_mb, int(capacity)
        self._lib = L.lib()
        h = C.c_void_p()
        L.check(self._lib.covahip_train_data_create(ctx.handle, h_mb, w_mb, self.capacity, C.byref(h)), "covahip_train_data_create",
                ctx.handle)
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            if getattr(self.ctx, "handle", None):
                self._lib.covahip_train_data_destroy(self.handle)
            self.handle = None

    __del__ = close

    @property
    def frames(self) -> int:
        n = C.c_int64()
        L.check(self._lib.covahip_train_data_frames(self.handle, C.byref(n)), "covahip_train_data_frames")
        return int(n.value)

    def _append(self, p_frames, p_gt, n, kind):
        first = C.c_int64()
        L.check(self._lib.covahip_train_data_append(self.handle, p_frames, p_gt, n, kind, C.byref(first)), "covahip_train_data_append",
                self.ctx.handle)
        return int(first.value), int(first.value) + n

    def append(self, frames: np.ndarray, gt: np.ndarray):
        """frames u8 [n][h][w][4] and gt u8 [n][h][w] of ONE contiguous recording; returns the half-open range of frame indices it
        filled: a segment (windows)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        gt = np.ascontiguousarray(gt, dtype=np.uint8)
        n = frames.shape[0]
        if frames.shape != (n, self.h, self.w, 4) or gt.shape != (n, self.h, self.w):
            raise ValueError(f"frames {frames.shape} / gt {gt.shape}: expected [n][{self.h}][{self.w}][4] and [n][{self.h}][{self.w}]")
        return self._append(frames.ctypes.data, gt.ctypes.data, n, L.MEM_HOST)

    def append_device(self, d_frames: int, d_gt: int, n: int):
        """The same from device pointers (packed by a kernel)."""
        return self._append(d_frames, d_gt, n, L.MEM_DEVICE)

    def set_stage(self, nbytes: int = 0) -> None:
        """Developer switch (include/covahip_dev.h): bytes of the staging of host appends and host-bound gathers, 0 = the default."""
        L.check(self._lib.covahip_dev_train_data_set_stage(self.handle, int(nbytes)), "covahip_dev_train_data_set_stage")

    def gather(self, samples):
        """(stacks u8 [n][4h][w][4], labels u8 [n][h][w]) of a SAMPLE array: the batch a step on these samples sees."""
        samples = _samples(samples)
        n = samples.shape[0]
        stack = np.empty((n, W.T * self.h, self.w, 4), np.uint8)
        gt = np.empty((n, self.h, self.w), np.uint8)
        L.check(self._lib.covahip_train_data_gather(self.handle, samples.ctypes.data, n, stack.ctypes.data, gt.ctypes.data, L.MEM_HOST),
                "covahip_train_data_gather", self.ctx.handle)
        return stack, gt

    def gather_device(self, samples, d_stack: int, d_gt: int) -> None:
        samples = _samples(samples)
        L.check(self._lib.covahip_train_data_gather(self.handle, samples.ctypes.data, samples.shape[0], d_stack, d_gt, L.MEM_DEVICE),
                "covahip_train_data_gather", self.ctx.handle)

    def _label_mass(self, first, n, keep, p_mass, kind):
        first = int(first)
        n = self.frames - first if n is None else int(n)
        if keep is not None:
            keep = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
            if keep.shape != (self.h, self.w):
                raise ValueError(f"keep must be [{self.h}][{self.w}], got {keep.shape}")
        mass = np.empty(max(n, 0), np.uint32) if p_mass is None else None
        L.check(self._lib.covahip_train_data_label_mass(self.handle, first, n, None if keep is None else keep.ctypes.data,
                                                        mass.ctypes.data if p_mass is None else p_mass, kind),
                "covahip_train_data_label_mass", self.ctx.handle)
        return mass

    def label_mass(self, first: int = 0, n: int | None = None, keep=None) -> np.ndarray:
        """u32 [n]: per frame of [first, first + n) (n None: up to `frames`) the number of macroblocks with a non-zero label
        byte, among those `keep` (u8 [h][w], non-zero = kept; None: all) keeps -- the label sum the loss of a camera with that
        ignore region sees, counted on the device (balanced_samples)."""
        return self._label_mass(first, n, keep, None, L.MEM_HOST)

    def record_stats(self, first: int | None = None, n: int | None = None) -> dict:
        """The input statistics of frames [first, first + n) (None: from 0 / up to `frames`), counted on the device
        (include/covahip.h, covahip_train_data_record_stats): in_frames, still_frames, intra_frames, set_total (ints), hist and
        hist_set i64 [512] (all records / the records at labelled macroblocks), moving i64 [h][w], move_hist i64 [16] -- the
        quantities cova_amd.monitor.read_inputs gives per served camera, so monitor.input_report(stats, None) reads them and
        monitor.save_inputs(path, stats, None) writes the baseline a deployed camera is compared with.  No keep map applies."""
        first = 0 if first is None else int(first)
        n = self.frames - first if n is None else int(n)
        one = {k: np.zeros(1, np.int64) for k in ("frames", "set_total", "still_frames", "intra_frames")}
        out = {"hist": np.zeros(L.INPUT_BINS, np.int64), "hist_set": np.zeros(L.INPUT_BINS, np.int64),
               "moving": np.zeros((self.h, self.w), np.int64), "move_hist": np.zeros(L.INPUT_MOVE_BINS, np.int64)}
        st = L.RecordStats(**{k: v.ctypes.data for k, v in {**one, **out}.items()})
        L.check(self._lib.covahip_train_data_record_stats(self.handle, first, n, C.byref(st)), "covahip_train_data_record_stats",
                self.ctx.handle)
        out.update(in_frames=int(one["frames"][0]), set_total=int(one["set_total"][0]), still_frames=int(one["still_frames"][0]),
                   intra_frames=int(one["intra_frames"][0]))
        return out

    def label_mass_device(self, d_mass: int, first: int = 0, n: int | None = None, keep=None) -> None:
        """The same into device memory: u32 [n] at d_mass, 4-byte aligned."""
        self._label_mass(first, n, keep, d_mass, L.MEM_DEVICE)

    def _align(self, first, n, max_shift, keep, min_mv, classes, ptrs, kind):
        first, n, max_shift = int(first), int(n), int(max_shift)
        if keep is not None:
            keep = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
            if keep.shape != (self.h, self.w):
                raise ValueError(f"keep must be [{self.h}][{self.w}], got {keep.shape}")
        mask = 0
        for c in classes:
            if not 0 <= int(c) <= 6:
                raise ValueError(f"classes = {tuple(classes)}: packed macroblock classes are 0 .. 6")
            mask |= 1 << int(c)
        out = None
        if ptrs is None:
            wide = 2 * max_shift + 1 if 0 <= max_shift <= 32 else 1    # a refused call writes nothing
            out = (np.empty((max(n, 0), wide), np.uint32), np.empty(max(n, 0), np.uint32), np.empty(max(n, 0), np.uint32))
            ptrs = [o.ctypes.data for o in out]
        cfg = L.AlignCfg(max_shift, int(min_mv), mask, None if keep is None else keep.ctypes.data)
        L.check(self._lib.covahip_train_data_align(self.handle, first, n, C.byref(cfg), ptrs[0], ptrs[1], ptrs[2], kind),
                "covahip_train_data_align", self.ctx.handle)
        return out

    def align(self, first: int, n: int, max_shift: int = 8, keep=None, min_mv: int = 1, classes=()):
        """(both u32 [n][2 S + 1], mov u32 [n], lab u32 [n]) of ONE recording, frames [first, first + n), S = max_shift, counted on
        the device (include/covahip.h, covahip_train_data_align): both[i][j] = the kept macroblocks that move in the records of
        frame first + i and are labelled in frame first + i + j - S (0 where that frame lies outside the recording), mov[i] and
        lab[i] the two counts on their own.  A macroblock moves when max(mv_x, mv_y) >= min_mv (0: the vectors decide nothing) or
        its packed class is among `classes`.  align_scores reads the three."""
        return self._align(first, n, max_shift, keep, min_mv, classes, None, L.MEM_HOST)

    def align_device(self, d_both: int, d_mov: int, d_lab: int, first: int, n: int, max_shift: int = 8, keep=None, min_mv: int = 1,
                     classes=()) -> None:
        """The same into device memory, each pointer 4-byte aligned."""
        self._align(first, n, max_shift, keep, min_mv, classes, [d_both, d_mov, d_lab], L.MEM_DEVICE)


def _align_sums(both, mov, lab, lo: int, hi: int):
    """Per shift (B, U) over the record frames i in [lo, hi) whose label frame i + s lies inside the recording, Python integers."""
    n, wide = both.shape
    S = wide // 2
    cm, cl = np.concatenate([[0], np.cumsum(mov, dtype=np.int64)]), np.concatenate([[0], np.cumsum(lab, dtype=np.int64)])
    out = []
    for s in range(-S, S + 1):
        a, b = max(lo, -s, 0), min(hi, n - s, n)
        if a >= b:
            out.append((0, 0))
            continue
        B = int(both[a:b, s + S].sum(dtype=np.int64))
        out.append((B, int(cm[b] - cm[a]) + int(cl[b + s] - cl[a + s]) - B))
    return out


def _align_best(sums):
    """The shift of largest B / U as exact fractions; ties: the smaller |s|, then the smaller s; None when every U is 0."""
    S = len(sums) // 2
    best = None
    for s in sorted(range(-S, S + 1), key=lambda v: (abs(v), v)):
        B, U = sums[s + S]
        if U > 0 and (best is None or B * sums[best + S][1] > sums[best + S][0] * U):
            best = s
    return best


def _align_arrays(both, mov, lab):
    both, mov, lab = np.asarray(both), np.asarray(mov).reshape(-1), np.asarray(lab).reshape(-1)
    if both.ndim != 2 or both.shape[1] % 2 != 1 or mov.shape != (both.shape[0],) or lab.shape != mov.shape:
        raise ValueError(f"both {both.shape}, mov {mov.shape}, lab {lab.shape}: expected [n][2 S + 1], [n] and [n]")
    return both, mov, lab


def align_scores(both, mov, lab) -> dict:
    """How well the labels of a recording sit on its records at every shift (TrainData.align's counts).  Per shift s, over the
    frames i with 0 <= i + s < n: B(s) = sum both[i][s + S], M(s) = sum mov[i], L(s) = sum lab[i + s], and the union
    U = M + L - B -- B / U is the overlap of "moves" and "labelled" as sets of (frame, macroblock).  Returns {"shifts", "B", "U"
    (lists, Python integers), "best"}: the shift of largest B / U compared as exact fractions; on ties the smaller |s|, then the
    smaller s; None when every U is 0.  s > 0: the label of record frame f stands at f + s (windows(label_shift=s))."""
    both, mov, lab = _align_arrays(both, mov, lab)
    sums = _align_sums(both, mov, lab, 0, both.shape[0])
    S = both.shape[1] // 2
    return {"shifts": list(range(-S, S + 1)), "B": [b for b, _ in sums], "U": [u for _, u in sums], "best": _align_best(sums)}


def align_drift(both, mov, lab, window: int = 256) -> dict:
    """align_scores' `best` per block of `window` record frames (the last block takes the remainder; a recording shorter than a
    window is one block), and the changes: [(first frame of the block, its shift)] for every block whose shift differs from the
    block before it that had one.  A frame lost in the middle of a recording shows as one change near the loss; a block in which
    no moving macroblock meets a labelled one at any shift (a quiet stretch) has no shift, None, and changes nothing.  Returns {"window", "best" (one per block),
    "changes"}; frames count from the recording's first."""
    both, mov, lab = _align_arrays(both, mov, lab)
    window = int(window)
    if window < 1:
        raise ValueError(f"window = {window}: at least one frame")
    n = both.shape[0]
    blocks = max(1, n // window)
    best, changes, last = [], [], None
    for b in range(blocks):
        lo, hi = b * window, n if b == blocks - 1 else (b + 1) * window
        sums = _align_sums(both, mov, lab, lo, hi)
        s = _align_best(sums)
        if s is not None and sums[s + both.shape[1] // 2][0] == 0:
            s = None                                                       # no macroblock in common at any shift
        best.append(s)
        if s is not None:
            if last is not None and s != last:
                changes.append((lo, s))
            last = s
    return {"window": window, "best": best, "changes": changes}


def alignment(data, segments, max_shift: int = 8, keep=None, min_mv: int = 1, classes=(), window: int = 256) -> list:
    """align_scores and align_drift of every segment (recording) of a TrainData: one dict per segment with "segment" (a, b),
    align_scores' entries and "drift" = align_drift's dict."""
    out = []
    for a, b in _segments(segments):
        counts = data.align(a, b - a, max_shift, keep, min_mv, classes)
        out.append({"segment": (a, b), **align_scores(*counts), "drift": align_drift(*counts, window)})
    return out


def _samples(samples) -> np.ndarray:
    samples = np.asarray(samples)
    if samples.dtype != SAMPLE or samples.ndim != 1:
        raise ValueError("samples: a one-dimensional array of dtype train.SAMPLE (epoch_samples, plain_samples)")
    return np.ascontiguousarray(samples)


def _pack_samples(per_model):
    """(SAMPLE array packed in model order, counts) of one SAMPLE array (or None) per model."""
    parts = [np.zeros(0, SAMPLE) if s is None else _samples(s) for s in per_model]
    return np.ascontiguousarray(np.concatenate(parts)), [int(p.shape[0]) for p in parts]


# ------------------------------------------------------------------------------------------------ GPU trainer
def set_epoch_plan(sizes, batch: int):
    """The steps of one epoch of a training set: a list of per-step lists [(start_k, count_k) for each model].  Model k walks
    its sizes[k] samples in order in batches of `batch`, the last one partial as in Keras; once its epoch is over it sits out
    the remaining steps with count 0.  The epoch has as many steps as the largest data set needs."""
    if batch < 1:
        raise ValueError("batch must be at least 1")
    if not sizes or min(sizes) < 1:
        raise ValueError("every model of a set needs at least one training sample")
    steps = max(-(-n // batch) for n in sizes)
    return [[(min(i * batch, n), max(0, min(batch, n - i * batch))) for n in sizes] for i in range(steps)]


class TrainerSet(_State):
    """K BlobNet models of one geometry trained side by side over covahip_train_create_set: a step takes one step of every
    model in one launch of each kernel.  Model k is bit-identical to a Trainer made from the same weights and seed and fed
    model k's steps alone (include/covahip.h, "Training sets")."""

    _tag_models = True      # fit's log lines name the model (a Trainer's set of one: they do not)

    def __init__(self, ctx, h_mb: int = 45, w_mb: int = 80, weights=None, n_models: int | None = None, seeds=None,
                 max_batch: int = 4, dropout: float = 0.2, lr: float = 1e-3, freeze=(), bn_inference=()):
        """weights: a list of flat weight arrays, one per model; or n_models with weights None: model k = init_weights(seeds[k]).
        seeds: the dropout seed per model (default 0, 1, ..).  freeze / bn_inference: the training plan (set_plan)."""
        plan_bits(freeze, bn_inference)             # a bad plan raises before anything is created
        if weights is None:
            if n_models is None:
                raise ValueError("TrainerSet needs weights=[...] or n_models=K")
            if seeds is None:
                seeds = list(range(n_models))
            weights = [init_weights(int(sd)) for sd in seeds]
        k = len(weights)
        if n_models is not None and n_models != k:
            raise ValueError(f"n_models = {n_models} but {k} weight arrays")
        if seeds is None:
            seeds = list(range(k))
        if len(seeds) != k:
            raise ValueError(f"{len(seeds)} seeds for {k} models")
        self.ctx, self.h, self.w, self.max_batch, self.n_models = ctx, h_mb, w_mb, max_batch, k
        self.seeds = [int(sd) for sd in seeds]
        self._lib = L.lib()
        cfg = L.TrainCfg()
        self._lib.covahip_train_default_cfg(C.byref(cfg))
        cfg.h_mb, cfg.w_mb, cfg.max_batch, cfg.dropout, cfg.lr = h_mb, w_mb, max_batch, dropout, lr
        cfg.seed = self.seeds[0] if k else 0
        self.cfg = cfg
        blobs = [W.to_bytes(w) for w in weights]
        ptrs = (C.c_char_p * max(1, k))(*blobs)
        sizes = (C.c_size_t * max(1, k))(*[len(b) for b in blobs])
        sd = (C.c_uint64 * max(1, k))(*self.seeds)
        h = C.c_void_p()
        L.check(self._lib.covahip_train_create_set(ctx.handle, C.byref(cfg), k, ptrs, sizes, sd, C.byref(h)),
                "covahip_train_create_set", ctx.handle)
        self.handle = h
        self.step_counts = [0] * k
        if freeze or bn_inference:
            self.set_plan(freeze, bn_inference)

    def close(self):
        if getattr(self, "handle", None):
            if getattr(self.ctx, "handle", None):      # (a trainer outliving its closed ctx is not freed)
                self._lib.covahip_train_destroy(self.handle)
            self.handle = None

    __del__ = close

    def _pack(self, pairs):
        """(stack, gt, counts) of one (stacks u8 [n_k][4h][w][4], labels u8 [n_k][h][w]) pair per model, packed in model order;
        a pair of None or of empty arrays counts 0."""
        xs, ys, counts = [], [], []
        for x, y in pairs:
            n = 0 if x is None else len(x)
            counts.append(n)
            if n:
                x = np.ascontiguousarray(x, dtype=np.uint8)
                y = np.ascontiguousarray(y, dtype=np.uint8)
                assert x.shape == (n, W.T * self.h, self.w, 4) and y.shape == (n, self.h, self.w), (x.shape, y.shape)
                xs.append(x)
                ys.append(y)
        if len(xs) == 1:
            return xs[0], ys[0], counts
        return np.concatenate(xs or [np.empty(0, np.uint8)]), np.concatenate(ys or [np.empty(0, np.uint8)]), counts

    def _lrs(self, lrs):
        if lrs is None:
            lrs = self.cfg.lr
        if np.isscalar(lrs):
            lrs = [lrs] * self.n_models
        if len(lrs) != self.n_models:
            raise ValueError(f"{len(lrs)} learning rates for {self.n_models} models")
        return np.ascontiguousarray(lrs, dtype=np.float32)

    def _step(self, p_stack, p_gt, batches, lrs, kind):
        batches = np.ascontiguousarray(batches, dtype=np.int32)
        if batches.shape != (self.n_models,):
            raise ValueError(f"{batches.size} batches for {self.n_models} models")
        lrs = self._lrs(lrs)
        losses = np.zeros(self.n_models, np.float32)
        L.check(self._lib.covahip_train_step_set(self.handle, p_stack, p_gt, batches.ctypes.data, lrs.ctypes.data,
                                                 losses.ctypes.data, kind), "covahip_train_step_set", self.ctx.handle)
        for k in range(self.n_models):
            self.step_counts[k] += int(batches[k] > 0)
        return [float(v) for v in losses]

    def step(self, stacks_per_model, labels_per_model, lrs=None):
        """One step of every model: stacks_per_model[k] u8 [b_k][4h][w][4] and labels_per_model[k] u8 [b_k][h][w]; an empty
        entry (or None) = model k sits this step out.  lrs: one rate for all, or one per model.  Returns the losses before
        the update (0 for a skipped model)."""
        if len(stacks_per_model) != self.n_models or len(labels_per_model) != self.n_models:
            raise ValueError(f"a step of this set takes {self.n_models} entries")
        stack, gt, batches = self._pack(zip(stacks_per_model, labels_per_model))
        if not any(batches):
            raise ValueError("a set step needs at least one model with samples")
        return self._step(stack.ctypes.data, gt.ctypes.data, batches, lrs, L.MEM_HOST)

    def step_device(self, d_stack: int, d_gt: int, batches, lrs=None):
        """The same on device pointers: the samples packed in model order (sum(batches) stacks, then as many labels)."""
        return self._step(d_stack, d_gt, batches, lrs, L.MEM_DEVICE)

    def metrics(self, k: int):
        """(TP, FP, FN) of model k's last step at sigmoid > 0.5; with a post, at its threshold over its keep map."""
        v = (C.c_int64 * 3)()
        L.check(self._lib.covahip_train_metrics_m(self.handle, k, v), "covahip_train_metrics_m")
        return int(v[0]), int(v[1]), int(v[2])

    def weights(self, k: int) -> np.ndarray:
        """Model k's current weights (moving statistics in the BN mean / var slots), flat."""
        return W.from_bytes(self.weights_bytes(k))

    def weights_bytes(self, k: int) -> bytes:
        n = C.c_size_t()
        rc = self._lib.covahip_train_weights_m(self.handle, k, None, 0, C.byref(n))
        if rc != 7:                                    # the size query answers COVAHIP_ERR_OVERFLOW (7); a bad k does not
            L.check(rc, "covahip_train_weights_m", self.ctx.handle)
        buf = np.zeros(n.value, np.uint8)
        L.check(self._lib.covahip_train_weights_m(self.handle, k, buf.ctypes.data, n.value, C.byref(n)), "covahip_train_weights_m",
                self.ctx.handle)
        return buf.tobytes()

    def grads(self, k: int) -> np.ndarray:
        """Model k's gradients of its last step, flat; BN mean / var slots = the batch mean / biased batch variance."""
        out = np.empty(W.N_PARAMS, np.float32)
        L.check(self._lib.covahip_train_grads_m(self.handle, k, out.ctypes.data, out.size), "covahip_train_grads_m", self.ctx.handle)
        return out

    def _set_step_counts(self, steps):
        self.step_counts = list(steps)

    def set_post(self, k: int, *, prob_thresh=None, logit_thresh=None, keep=None) -> None:
        """Model k's post from the next step or evaluation on (covahip_train_set_post), with the keywords of
        BlobNetInfer.set_post -- calibrate.load_post(path, h, w)[0] can be passed as **kw.  keep: u8 [h][w], non-zero = the
        macroblock takes part in the loss, its gradient and the metrics (None: all; see keep_from_rects).  The threshold, a
        probability or a logit (neither: 0), is where metrics() and evaluate() count a pixel as foreground: logit > threshold,
        serving's expression; the loss does not depend on it.  The post is not part of the trainer state: set it again after
        creating the trainer a state is loaded into."""
        from .elements import BlobNetInfer
        post = L.BlobNetPost(BlobNetInfer.post_logit_thresh(prob_thresh, logit_thresh), None)
        if keep is not None:
            keep = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
            if keep.shape != (self.h, self.w):
                raise ValueError(f"keep must be [{self.h}][{self.w}], got {keep.shape}")
            post.keep = keep.ctypes.data
        L.check(self._lib.covahip_train_set_post(self.handle, k, C.byref(post)), "covahip_train_set_post", self.ctx.handle)

    def reset_post(self, k: int) -> None:
        """Model k has no post again: the whole grid, and the metrics at sigmoid > 0.5."""
        L.check(self._lib.covahip_train_set_post(self.handle, k, None), "covahip_train_set_post", self.ctx.handle)

    def get_post(self, k: int):
        """Model k's post: (logit_thresh, keep u8 [h][w] of 0 / 1 -- all 1 without a keep map), or None without a post."""
        thr, has = C.c_float(), C.c_int()
        keep = np.empty((self.h, self.w), dtype=np.uint8)
        L.check(self._lib.covahip_train_get_post(self.handle, k, C.byref(thr), keep.ctypes.data, C.byref(has)), "covahip_train_get_post")
        return (thr.value, keep) if has.value else None

    def evaluate(self, records_per_model, want_sample_loss: bool = False, want_logits: bool = False):
        """Scores every model on its own samples in ONE call (one launch of each kernel per chunk of max_batch samples per
        model), in inference mode (moving BN statistics, no dropout); training does not notice.  records_per_model[k] =
        (stacks u8 [N_k][4h][w][4], labels u8 [N_k][h][w]) of model k, any size; None or an empty entry = nothing for model k
        (its dict holds zeros).  Returns one dict per model, {"loss", "precision", "recall", "iou", "samples"}: the mean
        per-sample Jaccard distance and the micro-averaged metrics at sigmoid > 0.5; plus "sample_loss" f32 [N_k] / "logits"
        f32 [N_k][h][w] when asked for.  Model k's is bit-identical to its evaluation alone."""
        if len(records_per_model) != self.n_models:
            raise ValueError(f"{len(records_per_model)} data sets for {self.n_models} models")
        stack, gt, counts = self._pack((None, None) if r is None else r for r in records_per_model)
        total = sum(counts)
        if not total:
            raise ValueError("no samples to evaluate: an evaluation needs at least one model with samples")
        sl = np.empty(total, np.float32) if want_sample_loss else None
        lg = np.empty((total, self.h, self.w), np.float32) if want_logits else None
        cnt = np.ascontiguousarray(counts, dtype=np.int32)
        res = (L.TrainEvalResult * self.n_models)()
        L.check(self._lib.covahip_train_eval_set(self.handle, stack.ctypes.data, gt.ctypes.data, cnt.ctypes.data,
                                                 None if sl is None else sl.ctypes.data, None if lg is None else lg.ctypes.data, res,
                                                 L.MEM_HOST), "covahip_train_eval_set", self.ctx.handle)
        outs, at = [], 0
        for k, n in enumerate(counts):
            outs.append(_eval_out(res[k], None if sl is None else sl[at:at + n], None if lg is None else lg[at:at + n]))
            at += n
        return outs

    def evaluate_device(self, d_stack: int, d_gt: int, counts, d_sample_loss: int | None = None, d_logits: int | None = None):
        """The same on device pointers: the samples packed in model order (sum(counts) stacks, then as many labels); the
        optional outputs are device buffers in the same packing."""
        cnt = np.ascontiguousarray(counts, dtype=np.int32)
        if cnt.shape != (self.n_models,):
            raise ValueError(f"{cnt.size} counts for {self.n_models} models")
        res = (L.TrainEvalResult * self.n_models)()
        L.check(self._lib.covahip_train_eval_set(self.handle, d_stack, d_gt, cnt.ctypes.data, d_sample_loss, d_logits, res,
                                                 L.MEM_DEVICE), "covahip_train_eval_set", self.ctx.handle)
        return [_eval_dict(r) for r in res]

    def best_weights_bytes(self, k: int) -> bytes:
        """Model k's weight file of ITS epoch with the lowest val_loss of the last fit(keep="best")."""
        if not getattr(self, "_best", None) or self._best[k] is None:
            raise ValueError("no best epoch: run fit(..., val=..., keep='best') first")
        return self._best[k][1]

    def fit(self, records_per_model, epochs: int = 20, batch: int = 4, schedule=keras_lr, log=None, val=None, keep: str = "last",
            checkpoint=None, start_epoch: int = 0):
        """records_per_model[k] = (stacks u8 [N][4h][w][4], labels u8 [N][h][w]) of model k (slide's output).  Every model walks
        its own data set in order (set_epoch_plan), the last batch partial as in Keras; a model whose epoch is shorter sits out
        the rest of it.  Returns one history per model: per epoch the sample-weighted mean loss and precision / recall at 0.5 of
        the training predictions.  Model k's weights afterwards are those of a fit on records_per_model[k] alone, bit for bit.
        val = one (stacks, labels) per model: every epoch record gains val_loss / val_precision / val_recall / val_iou (evaluate
        on val after the epoch).  keep="best": best_weights_bytes(k) returns model k's weights of its epoch with the lowest
        val_loss (ties: the earliest).  checkpoint=PATH: the trainer state is written there after every epoch (and the best
        epochs so far to PATH.best); load_state(PATH) returns the epoch to pass as start_epoch, which continues the schedule and
        the numbering: the histories returned then start at that epoch."""
        _check_fit_args(val, keep)
        if len(records_per_model) != self.n_models:
            raise ValueError(f"{len(records_per_model)} data sets for {self.n_models} models")
        if val is not None and len(val) != self.n_models:
            raise ValueError(f"{len(val)} validation sets for {self.n_models} models")
        if not 1 <= batch <= self.max_batch:
            raise ValueError(f"batch {batch} outside [1, max_batch = {self.max_batch}] of this trainer")
        sizes = [int(r[0].shape[0]) for r in records_per_model]
        if min(sizes) == 0:
            raise ValueError("no training samples")

        def take_step(ep, st, lr):
            xs = [records_per_model[k][0][a:a + n] for k, (a, n) in enumerate(st)]
            ys = [records_per_model[k][1][a:a + n] for k, (a, n) in enumerate(st)]
            return self.step(xs, ys, lr)

        return self._epochs(sizes, epochs, batch, schedule, log, keep, checkpoint, start_epoch, take_step,
                            None if val is None else lambda: self.evaluate(val))

    def _epochs(self, sizes, epochs, batch, schedule, log, keep, checkpoint, start_epoch, take_step, evaluate_val, note=""):
        """The epoch loop of fit and fit_data: take_step(epoch, step of set_epoch_plan, lr) -> losses; evaluate_val() -> one dict
        per model, or None for a run without validation; `note` ends every log line."""
        plan = set_epoch_plan(sizes, batch)
        self._best_start(self.n_models, keep, checkpoint, start_epoch)
        histories = [[] for _ in range(self.n_models)]
        for ep in range(start_epoch, epochs):
            lr = schedule(ep, self.cfg.lr) if schedule is keras_lr else schedule(ep)
            tot = [0.0] * self.n_models
            cnt = [[0, 0, 0] for _ in range(self.n_models)]
            for st in plan:
                losses = take_step(ep, st, lr)
                for k, (_, n) in enumerate(st):
                    if n:
                        tot[k] += losses[k] * n
                        for q, v in enumerate(self.metrics(k)):
                            cnt[k][q] += v
            evs = evaluate_val() if evaluate_val is not None else None
            for k in range(self.n_models):
                tp, fp, fn = cnt[k]
                rec = {"epoch": ep, "lr": lr, "loss": tot[k] / sizes[k], "precision": tp / max(1, tp + fp),
                       "recall": tp / max(1, tp + fn)}
                if evs is not None:
                    rec.update(_val_fields(evs[k]))
                    if keep == "best":
                        self._best_update(k, rec["val_loss"], functools.partial(self.weights_bytes, k))
                histories[k].append(rec)
                if log:
                    log(_epoch_text(ep, epochs, rec, k if self._tag_models else None) + (note and note.format(windows=sizes[k])))
            if checkpoint is not None:
                self.save_state(checkpoint, epoch=ep + 1)
                self._best_save(checkpoint)
        return histories

    # ---- the same from a resident data set (include/covahip.h, "Training data")
    def _check_data(self, data):
        if (data.h, data.w) != (self.h, self.w):
            raise ValueError(f"a {data.h}x{data.w} data set for a {self.h}x{self.w} trainer")

    def step_data(self, data, samples_per_model, lrs=None):
        """step() on samples of a TrainData: samples_per_model[k] = a SAMPLE array of b_k entries (None or empty: model k sits the
        step out).  Bit-identical to step() on data.gather() of the same samples."""
        if len(samples_per_model) != self.n_models:
            raise ValueError(f"a step of this set takes {self.n_models} entries")
        self._check_data(data)
        samples, batches = _pack_samples(samples_per_model)
        if not any(batches):
            raise ValueError("a set step needs at least one model with samples")
        bt = np.ascontiguousarray(batches, dtype=np.int32)
        lrs = self._lrs(lrs)
        losses = np.zeros(self.n_models, np.float32)
        L.check(self._lib.covahip_train_step_set_data(self.handle, data.handle, samples.ctypes.data, bt.ctypes.data, lrs.ctypes.data,
                                                      losses.ctypes.data), "covahip_train_step_set_data", self.ctx.handle)
        for k in range(self.n_models):
            self.step_counts[k] += int(batches[k] > 0)
        return [float(v) for v in losses]

    def evaluate_data(self, data, tables_per_model, stride: int = 1, want_sample_loss: bool = False, want_logits: bool = False):
        """evaluate() on windows of a TrainData: tables_per_model[k] = model k's windows() table, scored as they are (canonical
        order, forward, unmirrored, at `stride`), or a SAMPLE array to score exactly those samples; None or empty = nothing for
        model k.  Returns evaluate()'s dicts."""
        if len(tables_per_model) != self.n_models:
            raise ValueError(f"{len(tables_per_model)} tables for {self.n_models} models")
        self._check_data(data)
        per = [None if t is None else t if getattr(t, "dtype", None) == SAMPLE else plain_samples(t, stride) for t in tables_per_model]
        samples, counts = _pack_samples(per)
        total = sum(counts)
        if not total:
            raise ValueError("no samples to evaluate: an evaluation needs at least one model with samples")
        sl = np.empty(total, np.float32) if want_sample_loss else None
        lg = np.empty((total, self.h, self.w), np.float32) if want_logits else None
        cnt = np.ascontiguousarray(counts, dtype=np.int32)
        res = (L.TrainEvalResult * self.n_models)()
        L.check(self._lib.covahip_train_eval_set_data(self.handle, data.handle, samples.ctypes.data, cnt.ctypes.data,
                                                      None if sl is None else sl.ctypes.data, None if lg is None else lg.ctypes.data,
                                                      res, L.MEM_HOST), "covahip_train_eval_set_data", self.ctx.handle)
        outs, at = [], 0
        for k, n in enumerate(counts):
            outs.append(_eval_out(res[k], None if sl is None else sl[at:at + n], None if lg is None else lg[at:at + n]))
            at += n
        return outs

    def _masses(self, data, tables, balance, log, shifts):
        """fit_data(balance=...): per model (first frame, label mass of the frames its table's labels span, under its post's keep map)."""
        out = []
        for k, t in enumerate(tables):
            sh = np.broadcast_to(np.asarray(shifts[k], dtype=np.int64), (t.shape[0],))
            lo, hi = int((t[:, 0] + np.minimum(sh, 0)).min()), int((t[:, 1] + np.maximum(sh, 0)).max()) + 1
            post = self.get_post(k)
            keep = None if post is None or post[1].all() else post[1]
            mass = data.label_mass(lo, hi - lo, keep)
            busy = int((mass[t[:, 1] + sh - lo] >= balance).sum())
            if log:
                log(f"{f'model {k}: ' if self._tag_models else ''}balance {balance}: {busy} busy / {t.shape[0] - busy} quiet windows")
            out.append((lo, mass))
        return out

    def fit_data(self, data, tables_per_model, epochs: int = 20, batch: int = 4, *, strides=(1,), shuffle: bool = False, flip=(),
                 reverse: bool = False, data_seed: int = 0, val_tables=None, schedule=keras_lr, log=None, keep: str = "last",
                 checkpoint=None, start_epoch: int = 0, balance: int | None = None, label_shift=None):
        """fit() from a resident TrainData: tables_per_model[k] = model k's windows() table, and every epoch walks
        epoch_samples(table, strides, data_seed, epoch, model = k, shuffle, flip, reverse) of it -- a new order and new mirrors
        every epoch, a pure function of (data_seed, epoch, k), so a resumed run continues exactly.  Everything else is fit's:
        set_epoch_plan, the partial last batch, the histories, keep="best", the checkpoints.  val_tables = one table per model,
        scored after every epoch as they are, at min(strides), never shuffled or augmented.  With windows(mode="skip") and no
        augmentation this is fit(slide(...)), bit for bit.  The augmentation settings are not part of the checkpoint: a resumed
        run passes them again, like the plan and the post.
        balance = a label-mass threshold (the reference's 100 at 45x80): every epoch becomes balanced_samples(epoch_samples(...),
        mass, balance, ...) with the same data_seed, epoch and model -- as many samples, half of the draws busy.  Model k's masses
        are taken once, before the first epoch, under the keep map of ITS post if it has one (TrainData.label_mass), and the
        log gains one line per model with the busy / quiet windows of its table (each classed by its newest frame, the label of
        the forward window).  Validation tables are never balanced.  Like the augmentation settings `balance` is not in the
        checkpoint; None runs exactly what ran before the keyword existed.
        label_shift = one entry per model, epoch_samples' label_shift for that model's table (a shift, or one per row; the
        tables come from windows(label_shift=...)); None is 0 everywhere.  A validation table that needs a shift is passed as
        the SAMPLE array epoch_samples(table, (min(strides),), label_shift=...) makes of it."""
        _check_fit_args(val_tables, keep)
        if len(tables_per_model) != self.n_models:
            raise ValueError(f"{len(tables_per_model)} tables for {self.n_models} models")
        if val_tables is not None and len(val_tables) != self.n_models:
            raise ValueError(f"{len(val_tables)} validation tables for {self.n_models} models")
        if not 1 <= batch <= self.max_batch:
            raise ValueError(f"batch {batch} outside [1, max_batch = {self.max_batch}] of this trainer")
        self._check_data(data)
        strides = _strides(strides)
        tables = [np.asarray(t, dtype=np.int64).reshape(-1, 2) for t in tables_per_model]
        sizes = [int(t.shape[0]) for t in tables]
        if min(sizes) == 0:
            raise ValueError("no training samples")
        current = {}
        shifts = [0] * self.n_models if label_shift is None else list(label_shift)
        if len(shifts) != self.n_models:
            raise ValueError(f"{len(shifts)} label shifts for {self.n_models} models")
        masses = None if balance is None else self._masses(data, tables, balance, log, shifts)

        def take_step(ep, st, lr):
            if current.get("epoch") != ep:
                current["epoch"] = ep
                current["samples"] = [epoch_samples(t, strides, data_seed, ep, k, shuffle, flip, reverse, shifts[k])
                                      for k, t in enumerate(tables)]
                if masses is not None:
                    current["samples"] = [balanced_samples(s, mass, balance, mass_first=lo, data_seed=data_seed, epoch=ep, model=k)
                                          for k, (s, (lo, mass)) in enumerate(zip(current["samples"], masses))]
            return self.step_data(data, [current["samples"][k][a:a + n] for k, (a, n) in enumerate(st)], lr)

        return self._epochs(sizes, epochs, batch, schedule, log, keep, checkpoint, start_epoch, take_step,
                            None if val_tables is None else lambda: self.evaluate_data(data, val_tables, min(strides)),
                            note=" windows {windows}")


class Trainer(_State):
    """One BlobNet trained on the GPU: a TrainerSet of one model, with its lists of one unwrapped.  `step_count` counts the
    steps taken (the dropout hash's step)."""

    def __init__(self, ctx, h_mb: int = 45, w_mb: int = 80, max_batch: int = 4, weights_flat: np.ndarray | None = None,
                 seed: int = 0, dropout: float = 0.2, lr: float = 1e-3, freeze=(), bn_inference=()):
        self._set = s = TrainerSet(ctx, h_mb, w_mb, [init_weights(seed) if weights_flat is None else weights_flat], seeds=[seed],
                                   max_batch=max_batch, dropout=dropout, lr=lr, freeze=freeze, bn_inference=bn_inference)
        s._tag_models = False
        self.ctx, self.h, self.w, self.max_batch, self.cfg, self._lib = ctx, h_mb, w_mb, max_batch, s.cfg, s._lib

    handle = property(lambda self: self._set.handle)
    step_count = property(lambda self: self._set.step_counts[0])

    def close(self):
        if getattr(self, "_set", None):
            self._set.close()

    __del__ = close

    def _set_step_counts(self, steps):
        self._set._set_step_counts(steps)

    def set_post(self, *, prob_thresh=None, logit_thresh=None, keep=None) -> None:
        """TrainerSet.set_post of the one model."""
        self._set.set_post(0, prob_thresh=prob_thresh, logit_thresh=logit_thresh, keep=keep)

    def reset_post(self) -> None:
        self._set.reset_post(0)

    def get_post(self):
        """(logit_thresh, keep u8 [h][w]) or None without a post."""
        return self._set.get_post(0)

    def step(self, stack: np.ndarray, gt: np.ndarray, lr: float | None = None) -> float:
        """One training step on stack u8 [B][4h][w][4] with labels u8 [B][h][w]; returns the loss before the update."""
        stack, gt, batches = self._set._pack([(stack, gt)])
        return self._set._step(stack.ctypes.data, gt.ctypes.data, batches, lr, L.MEM_HOST)[0]

    def step_device(self, d_stack: int, d_gt: int, batch: int, lr: float | None = None) -> float:
        """The same on device pointers (stack u8 [batch][4h][w][4], labels u8 [batch][h][w] on the ctx's GPU)."""
        return self._set.step_device(d_stack, d_gt, [batch], lr)[0]

    def metrics(self):
        """(TP, FP, FN) of the last step at sigmoid > 0.5."""
        return self._set.metrics(0)

    def weights(self) -> np.ndarray:
        """The current weights (moving statistics in the BN mean / var slots), flat."""
        return self._set.weights(0)

    def weights_bytes(self) -> bytes:
        return self._set.weights_bytes(0)

    def grads(self) -> np.ndarray:
        """The last step's gradients, flat; BN mean / var slots = the batch mean / biased batch variance."""
        return self._set.grads(0)

    def evaluate(self, records, want_sample_loss: bool = False, want_logits: bool = False) -> dict:
        """TrainerSet.evaluate of records = (stacks, labels), any N >= 1: the one dict."""
        return self._set.evaluate([records], want_sample_loss, want_logits)[0]

    def evaluate_device(self, d_stack: int, d_gt: int, n: int, d_sample_loss: int | None = None, d_logits: int | None = None) -> dict:
        """The same on device pointers (the optional outputs are device buffers of n and n * h * w floats)."""
        return self._set.evaluate_device(d_stack, d_gt, [n], d_sample_loss, d_logits)[0]

    def best_weights_bytes(self) -> bytes:
        """The weight file of the epoch with the lowest val_loss of the last fit(keep="best")."""
        return self._set.best_weights_bytes(0)

    def fit(self, records, epochs: int = 20, batch: int = 4, schedule=keras_lr, log=None, val=None, keep: str = "last",
            checkpoint=None, start_epoch: int = 0):
        """TrainerSet.fit of records = (stacks, labels) and val = (stacks, labels) or None: the one history."""
        return self._set.fit([records], epochs, batch, schedule, log, None if val is None else [val], keep, checkpoint, start_epoch)[0]

    def step_data(self, data, samples, lr: float | None = None) -> float:
        """TrainerSet.step_data of the one model: a SAMPLE array of the batch."""
        return self._set.step_data(data, [samples], lr)[0]

    def evaluate_data(self, data, table, stride: int = 1, want_sample_loss: bool = False, want_logits: bool = False) -> dict:
        """TrainerSet.evaluate_data of the one table (or SAMPLE array): the one dict."""
        return self._set.evaluate_data(data, [table], stride, want_sample_loss, want_logits)[0]

    def fit_data(self, data, table, epochs: int = 20, batch: int = 4, *, val_table=None, **kw):
        """TrainerSet.fit_data of the one table and val_table (or None), with its keywords: the one history."""
        if kw.get("label_shift") is not None:
            kw["label_shift"] = [kw["label_shift"]]
        return self._set.fit_data(data, [table], epochs, batch, val_tables=None if val_table is None else [val_table], **kw)[0]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cova_amd.train", description=__doc__.split("\n")[0])
    ap.add_argument("records", nargs="+", help="TFRecord files written by tfrecordsink gt=LABELS; with --set one model per "
                                               "argument, several files of one model joined with commas")
    ap.add_argument("-o", "--output", help="weight file to write (CVHW); with --set the directory for one file per model")
    ap.add_argument("--set", action="store_true", dest="as_set", help="train one model per argument in one training set")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--h-mb", type=int, default=45)
    ap.add_argument("--w-mb", type=int, default=80)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--val", nargs="+", metavar="FILES", help="validation records; with --set one comma-joined argument per model, "
                                                              "in model order")
    ap.add_argument("--val-frac", type=float, metavar="F", help="validate on the last ceil(F * N) samples (of every model) instead")
    ap.add_argument("--keep", choices=("last", "best"), default="last", help="which epoch's weights to write: the last, or the one "
                                                                             "with the lowest validation loss")
    ap.add_argument("--checkpoint", metavar="PATH", help="write the trainer state here after every epoch")
    ap.add_argument("--resume", metavar="PATH", help="load a trainer state and continue at its epoch, up to --epochs")
    ap.add_argument("--eval-only", metavar="WEIGHTS", help="train nothing: score this weight file (with --set: a directory of "
                                                           "weight files named as --set writes them) on the records, one JSON "
                                                           "line per model")
    ap.add_argument("--init", metavar="WEIGHTS", help="start from this weight file instead of a fresh initialisation (with --set: "
                                                      "one file for every model, or a directory of per-model files named as "
                                                      "--set -o writes them)")
    ap.add_argument("--freeze", metavar="GROUPS", help="layer groups that are not trained: enc0..enc3, dec0..dec3 joined with "
                                                       "commas, or encoder / decoder")
    ap.add_argument("--freeze-bn", action="store_true", help="every BatchNorm layer normalises with its moving statistics and "
                                                             "leaves them alone")
    ap.add_argument("--post", metavar="FILE", help="the camera's calibration sidecar (python -m cova_amd.calibrate -o): train and "
                                                   "score with its ignore region and mask threshold (with --set: one file for "
                                                   "every model, or a directory of <stem>.json per model, named as --set -o names "
                                                   "weight files)")
    ap.add_argument("--math", choices=MATH_MODES, default="exact", help="the arithmetic of the convolutions: 'exact', the plain "
                                                                        "kernels, or 'matrix', fp32 implicit GEMMs on the "
                                                                        "matrix cores (faster; bit-reproducible within the "
                                                                        "mode, not against 'exact')")
    ap.add_argument("--ignore-rects", type=_rects, metavar="L,T,W,H[+...]", help="pixel rectangles of the camera's ignore region, "
                                                                                 "for a camera without a sidecar")
    ap.add_argument("--mask-threshold", type=float, metavar="P", help="the camera's mask threshold as a probability, for a camera "
                                                                      "without a sidecar")
    ap.add_argument("--windows", choices=("skip", "overlap"), help="which windows of a recording are samples: 'skip', frames "
                                                                   "4j..4j+3 (what runs without these flags), or 'overlap', "
                                                                   "every window: F - 3 of F frames.  This and the five flags "
                                                                   "below train from a device-resident data set, each file one "
                                                                   "segment that no window crosses")
    ap.add_argument("--stride", type=_stride_list, metavar="S[,S...]", help="frame strides of a window, one drawn per sample and epoch")
    ap.add_argument("--flip", choices=("x", "y", "xy"), help="mirror samples in x, y or both, drawn per sample and epoch")
    ap.add_argument("--reverse", action="store_true", help="reverse samples in time, drawn per sample and epoch")
    ap.add_argument("--shuffle", action="store_true", help="a new sample order every epoch")
    ap.add_argument("--data-seed", type=int, metavar="N", help="seed of the order and the augmentation draws (default 0)")
    ap.add_argument("--balance", type=int, metavar="N", help="draw every epoch half from the busy windows, whose labelling frame "
                                                             "carries at least N labelled macroblocks the camera keeps, and half "
                                                             "from the quiet ones (the reference's utils/data/balance.py: 100 at "
                                                             "45x80); trains from the device-resident data set")
    ap.add_argument("--align-report", type=int, nargs="?", const=8, metavar="S", help="train nothing: score every recording's labels "
                    "against its records at the frame shifts -S .. S (default 8, at most 32) on the device-resident data set, "
                    "print the table (shift, B, U, B/U) and the frames where the best shift changes, and exit; needs --windows")
    ap.add_argument("--label-shift", type=_label_shift, metavar="N|auto[:S]", help="label every window by its labelling frame + N; "
                    "'auto' measures every recording's own shift (within -S .. S, default 8) and stops when a recording has "
                    "none, has it at the edge of the range, or changes it half-way; needs --windows")
    ap.add_argument("--record-report", action="store_true", help="train nothing: per recording, count the records on the "
                    "device-resident data set and print the class and vector marginals, the GoP estimate, the still share, the share "
                    "of labelled macroblocks whose record is all skip and the share of moving macroblocks that are labelled, and "
                    "exit; needs --windows")
    ap.add_argument("--save-inputs", nargs="+", metavar="JSON", help="with --record-report: write the input counts of all of a "
                    "model's recordings together, one file per model -- the training baseline python -m cova_amd.monitor "
                    "--input-baseline compares a deployed camera with")
    ap.add_argument("--align-window", type=int, default=256, metavar="F", help="frames of a block of the drift list (default 256)")
    a = ap.parse_args(argv)
    a.resident = (a.windows is not None or a.stride is not None or a.flip is not None or a.reverse or a.shuffle
                  or a.data_seed is not None or a.balance is not None)
    if (a.align_report is not None or a.label_shift is not None) and a.windows is None:
        ap.error("--align-report / --label-shift read the device-resident data set: give --windows skip|overlap")
    if a.record_report and a.windows is None:
        ap.error("--record-report reads the device-resident data set: give --windows skip|overlap")
    if a.save_inputs and not a.record_report:
        ap.error("--save-inputs writes what --record-report counts")
    if a.save_inputs and len(a.save_inputs) != (len(a.records) if a.as_set else 1):
        ap.error("--save-inputs takes one file per model")
    if a.align_report is not None and not 0 <= a.align_report <= 32:
        ap.error("--align-report scores the shifts -S .. S, 0 <= S <= 32")
    if a.align_window < 1:
        ap.error("--align-window is a count of frames, at least 1")
    if a.eval_only and a.balance is not None:
        ap.error("--balance shapes a training's epochs; --eval-only scores every window once")
    if a.balance is not None and a.balance < 1:
        ap.error("--balance is a count of macroblocks, at least 1")
    if a.eval_only and (a.flip or a.reverse or a.shuffle or a.data_seed is not None):
        ap.error("--flip / --reverse / --shuffle / --data-seed shape a training; --eval-only trains nothing")
    if a.eval_only and a.stride is not None and len(a.stride) != 1:
        ap.error("--eval-only scores every window at ONE stride: --stride S")
    if a.post and (a.ignore_rects is not None or a.mask_threshold is not None):
        ap.error("--post carries the ignore region and the threshold: it excludes --ignore-rects and --mask-threshold")
    if a.mask_threshold is not None and not 0.0 < a.mask_threshold < 1.0:
        ap.error("--mask-threshold is a probability strictly between 0 and 1")
    if a.post:
        try:
            post_paths(a.records if a.as_set else None, a.post)
        except ValueError as e:
            ap.error(str(e))
    if a.align_report is not None or a.record_report:
        return a
    if a.eval_only:
        if a.resume:
            ap.error("--resume continues a training; --eval-only trains nothing")
        if a.init or a.freeze or a.freeze_bn:
            ap.error("--init / --freeze / --freeze-bn shape a training; --eval-only trains nothing")
        if a.val or a.val_frac is not None or a.checkpoint or a.keep != "last" or a.output:
            ap.error("--eval-only takes the weights and the records only")
        return a
    if not a.output:
        ap.error("-o / --output is required")
    if a.val and a.val_frac is not None:
        ap.error("--val and --val-frac exclude each other")
    if a.keep == "best" and not a.val and a.val_frac is None:
        ap.error("--keep best needs validation data: --val FILES or --val-frac F")
    if a.val_frac is not None and not 0.0 < a.val_frac < 1.0:
        ap.error("--val-frac must lie strictly between 0 and 1")
    if a.val and a.as_set and len(a.val) != len(a.records):
        ap.error(f"--val names {len(a.val)} models, the set has {len(a.records)}")
    if a.init and a.resume:
        ap.error("--init and --resume exclude each other: a checkpoint holds its own weights")
    try:
        plan_bits(a.freeze, "all" if a.freeze_bn else ())
    except ValueError as e:
        ap.error(str(e))
    return a


def _stride_list(text):
    """--stride: S[,S...], each at least 1."""
    try:
        return _strides([int(v) for v in text.split(",")])
    except ValueError:
        raise argparse.ArgumentTypeError(f"strides are positive integers joined with commas, got {text!r}")


def _label_shift(text):
    """--label-shift: an integer, or auto[:S] as ("auto", S) with 1 <= S <= 32."""
    try:
        if text == "auto" or text.startswith("auto:"):
            S = int(text[5:]) if text != "auto" else 8
            if not 1 <= S <= 32:
                raise ValueError
            return ("auto", S)
        return int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"a frame shift N, or auto[:S] with S in 1 .. 32, got {text!r}")


def _rects(text):
    """--ignore-rects: L,T,W,H[+L,T,W,H...] in pixels, as blobnetfilter's pad-ignore-rects writes them."""
    out = []
    for part in text.split("+"):
        try:
            vals = [int(v) for v in part.split(",")]
        except ValueError:
            vals = []
        if len(vals) != 4:
            raise argparse.ArgumentTypeError(f"a rectangle is LEFT,TOP,WIDTH,HEIGHT in pixels, got {part!r}")
        out.append(tuple(vals))
    return out


def post_paths(records, post: str):
    """--post: the sidecar of every model, in argument order (records None: the one model of a run without --set).  A file
    serves every model; a directory (--set only) holds <stem>.json per model, named as --set -o names weight files (set_jobs).
    A missing file is a ValueError."""
    if not os.path.isdir(post):
        if not os.path.isfile(post):
            raise ValueError(f"--post {post}: no such file")
        return [post] * (1 if records is None else len(records))
    if records is None:
        raise ValueError(f"--post {post}: a directory of sidecars needs --set")
    paths = [os.path.splitext(p)[0] + ".json" for _, p in set_jobs(records, post)]
    missing = [p for p in paths if not os.path.isfile(p)]
    if missing:
        raise ValueError(f"--post {post}: no sidecar {', '.join(missing)}")
    return paths


def post_settings(a, n_models: int):
    """The set_post keywords of every model from --post, or from --ignore-rects / --mask-threshold (the same for every model);
    None when the command line names no post."""
    if a.post:
        from .calibrate import load_post
        return [load_post(p, a.h_mb, a.w_mb)[0] for p in post_paths(a.records if a.as_set else None, a.post)]
    if a.ignore_rects is None and a.mask_threshold is None:
        return None
    from .elements import keep_from_rects
    kw = {"prob_thresh": a.mask_threshold, "keep": keep_from_rects(a.h_mb, a.w_mb, a.ignore_rects) if a.ignore_rects else None}
    return [kw] * n_models


def _apply_posts(trainer, posts) -> None:
    """posts (post_settings) onto a TrainerSet, or onto a Trainer's one model."""
    if posts is not None:
        for k, kw in enumerate(posts):
            getattr(trainer, "_set", trainer).set_post(k, **kw)


def _plan_kw(a) -> dict:
    """The Trainer / TrainerSet keywords of --freeze / --freeze-bn."""
    return {"freeze": a.freeze or (), "bn_inference": "all" if a.freeze_bn else ()}


def _read_weights(path) -> np.ndarray:
    with open(path, "rb") as f:
        return W.from_bytes(f.read())


def init_paths(records, init: str):
    """--init with --set: the weight file of every model, in argument order.  A directory holds one file per model, named as
    --set -o names them (set_jobs); a file initialises every model.  A missing per-model file is a ValueError."""
    if not os.path.isdir(init):
        return [init] * len(records)
    paths = [p for _, p in set_jobs(records, init)]
    missing = [p for p in paths if not os.path.isfile(p)]
    if missing:
        raise ValueError(f"--init {init}: no weight file {', '.join(missing)}")
    return paths


def _load(files, a):
    frames, gt = read_tfrecords(files, a.h_mb, a.w_mb)
    return frames.shape[0], slide(frames, gt)


def _resume(trainer, a, n_models: int) -> int:
    """--resume: the stored epoch, after the state has been loaded into `trainer`."""
    if not a.resume:
        return 0
    with open(a.resume, "rb") as f:
        data = f.read()
    hdr = read_state_header(data)
    if (hdr["h_mb"], hdr["w_mb"], hdr["n_models"]) != (a.h_mb, a.w_mb, n_models):
        raise ValueError(f"{a.resume}: state of {hdr['n_models']} model(s) at {hdr['h_mb']}x{hdr['w_mb']}, this run trains "
                         f"{n_models} at {a.h_mb}x{a.w_mb}")
    epoch = trainer.load_state_bytes(data)
    print(f"resumed {a.resume}: continuing at epoch {epoch + 1}/{a.epochs}", file=sys.stderr)
    return epoch


def main_eval(a) -> int:
    from .elements import Context

    if a.as_set:
        jobs = set_jobs(a.records, a.eval_only)
    else:
        jobs = [(a.records, a.eval_only)]
    flats, records = [], []
    for files, path in jobs:
        with open(path, "rb") as f:
            flats.append(W.from_bytes(f.read()))
        records.append(_load(files, a)[1])
    posts = post_settings(a, len(jobs))
    ctx = Context(a.device)
    if a.as_set:
        ts = TrainerSet(ctx, a.h_mb, a.w_mb, weights=flats, max_batch=a.batch)
        _apply_posts(ts, posts)
        ts.set_math(a.math)
        evs = ts.evaluate(records)
    else:
        ts = Trainer(ctx, a.h_mb, a.w_mb, max_batch=a.batch, weights_flat=flats[0])
        _apply_posts(ts, posts)
        ts.set_math(a.math)
        evs = [ts.evaluate(records[0])]
    for k, ((_, path), ev) in enumerate(zip(jobs, evs)):
        if posts is not None:
            thr, keep = getattr(ts, "_set", ts).get_post(k)
            ev["post"] = {"logit_thresh": thr, "ignored": int((keep == 0).sum())}
        print(json.dumps({"weights": path, **ev}))
    ts.close()
    ctx.close()
    return 0


def set_jobs(records, outdir: str):
    """--set: [(files of model k, its output path)] in argument order.  A model's output is OUTDIR/<stem of its first file>.cvhw;
    two models that would share a name are an error."""
    jobs, seen = [], set()
    for arg in records:
        files = [f for f in arg.split(",") if f]
        if not files:
            raise ValueError(f"empty model argument {arg!r}")
        stem = os.path.splitext(os.path.basename(files[0]))[0]
        if stem in seen:
            raise ValueError(f"two models would be written to {stem}.cvhw")
        seen.add(stem)
        jobs.append((files, os.path.join(outdir, stem + ".cvhw")))
    return jobs


def main_set(a) -> int:
    from .elements import Context

    jobs = set_jobs(a.records, a.output)
    records, val = [], ([] if a.val or a.val_frac is not None else None)
    for k, (files, _) in enumerate(jobs):
        n_frames, rec = _load(files, a)
        if a.val:
            val.append(_load([f for f in a.val[k].split(",") if f], a)[1])
        elif a.val_frac is not None:
            rec, v = split_tail(*rec, a.val_frac)
            val.append(v)
        records.append(rec)
        print(f"model {k}: {n_frames} frames -> {rec[0].shape[0]} samples of {a.h_mb}x{a.w_mb}"
              + (f", {val[k][0].shape[0]} to validate" if val is not None else ""), file=sys.stderr)
    os.makedirs(a.output, exist_ok=True)
    posts = post_settings(a, len(jobs))
    ctx = Context(a.device)
    init = [_read_weights(p) for p in init_paths(a.records, a.init)] if a.init else None
    ts = TrainerSet(ctx, a.h_mb, a.w_mb, weights=init, n_models=len(jobs), seeds=[a.seed + k for k in range(len(jobs))],
                    max_batch=a.batch, **_plan_kw(a))
    _apply_posts(ts, posts)
    ts.set_math(a.math)
    start = _resume(ts, a, len(jobs))
    ts.fit(records, epochs=a.epochs, batch=a.batch, log=lambda s: print(s, file=sys.stderr), val=val, keep=a.keep,
           checkpoint=a.checkpoint, start_epoch=start)
    for k, (_, out) in enumerate(jobs):
        with open(out, "wb") as f:
            f.write(ts.best_weights_bytes(k) if a.keep == "best" else ts.weights_bytes(k))
    ts.close()
    ctx.close()
    return 0


def align_report_text(name: str, rec: dict) -> str:
    """--align-report: one recording's alignment() entry as text -- the table (shift, B, U, B/U) and the drift list."""
    a, b = rec["segment"]
    best = rec["best"]
    lines = [f"{name}: frames [{a}, {b}), best shift {'none' if best is None else format(best, '+d')}",
             f"  {'shift':>5} {'B':>12} {'U':>12} {'B/U':>8}"]
    for s, B, U in zip(rec["shifts"], rec["B"], rec["U"]):
        lines.append(f"  {s:>+5d} {B:>12d} {U:>12d} {(B / U if U else 0.0):>8.4f}" + (" *" if s == best else ""))
    ch = rec["drift"]["changes"]
    lines.append(f"  drift (blocks of {rec['drift']['window']} frames): " +
                 ("none" if not ch else ", ".join(f"frame {a + f}: shift {s:+d}" for f, s in ch)))
    return "\n".join(lines)


def auto_label_shift(name: str, rec: dict) -> int:
    """--label-shift auto: the recording's `best`, or a ValueError naming the recording and the frames when one offset cannot be
    trusted to fix it: no shift at all, the best at the edge of the range (the peak may lie outside), or a drift list."""
    a, b = rec["segment"]
    S, best, ch = rec["shifts"][-1], rec["best"], rec["drift"]["changes"]
    where = f"--label-shift auto: {name}, frames [{a}, {b})"
    if best is None:
        raise ValueError(f"{where}: nothing moves and nothing is labelled, there is no shift to measure")
    if abs(best) == S:
        raise ValueError(f"{where}: the best shift {best:+d} sits at the edge of -{S} .. {S}; the peak may lie outside, try auto:{min(2 * S, 32)}")
    if ch:
        raise ValueError(f"{where}: the shift changes inside the recording (" + ", ".join(f"frame {a + f}: {s:+d}" for f, s in ch) +
                         "); one offset cannot fix a recording that lost a frame half-way, cut it there")
    return best


def record_report_text(name: str, st: dict) -> str:
    """--record-report: one recording's TrainData.record_stats as text."""
    from . import monitor
    rep = monitor.input_report(st, None)
    r = np.arange(L.INPUT_BINS)
    total, moving = rep["macroblocks"], int(np.asarray(st["hist"])[(r & 0x1F8) != 0].sum())
    set_moving = int(np.asarray(st["hist_set"])[(r & 0x1F8) != 0].sum())
    skip_share = "n/a" if not st["set_total"] else f"{100.0 * int(st['hist_set'][0]) / st['set_total']:.2f} %"
    lab_share = "n/a" if not moving else f"{100.0 * set_moving / moving:.2f} %"
    return (monitor.format_input_report(rep, name) +
            f"\n  labelled macroblocks {st['set_total']} of {total}: all-skip records among them {skip_share}; "
            f"moving macroblocks that are labelled {lab_share}")


def _record_report(a, data, recs, k):
    """--record-report for model k's recordings [(name, (first, end))]; --save-inputs: their counts together."""
    from . import monitor
    total = None
    for name, (lo, hi) in recs:
        st = data.record_stats(lo, hi - lo)
        print(record_report_text(name, st))
        total = st if total is None else {key: total[key] + st[key] for key in st}
    if a.save_inputs and total is not None:
        monitor.save_inputs(a.save_inputs[k], total, None)
        print(f"wrote {a.save_inputs[k]}")


def _recording_shifts(a, data, recs, keep):
    """[(first, end, shift)] of one model's recordings [(name, (first, end))] under --label-shift; --align-report prints instead."""
    if a.align_report is None and not isinstance(a.label_shift, tuple):
        return [(lo, hi, a.label_shift or 0) for _, (lo, hi) in recs]
    S = a.align_report if a.align_report is not None else a.label_shift[1]
    found = alignment(data, [seg for _, seg in recs], S, keep, window=a.align_window)
    if a.align_report is not None:
        for (name, _), rec in zip(recs, found):
            print(align_report_text(name, rec))
        return None
    out = []
    for (name, (lo, hi)), rec in zip(recs, found):
        out.append((lo, hi, auto_label_shift(name, rec)))
        print(f"{name}: label shift {out[-1][2]:+d}", file=sys.stderr)
    return out


def _shifted_windows(segs, rec_shifts, mode, strides):
    """(table, shift per row) of segments that each lie inside one of the recordings [(first, end, shift)]."""
    tabs, rows = [np.zeros((0, 2), np.int64)], [np.zeros(0, np.int64)]
    for lo, hi in segs:
        s = next(sh for ra, rb, sh in rec_shifts if ra <= lo and hi <= rb)
        tabs.append(windows([(lo, hi)], mode, strides, s))
        rows.append(np.full(tabs[-1].shape[0], s, np.int64))
    return np.concatenate(tabs), np.concatenate(rows)


def main_resident(a) -> int:
    """Training or scoring from a device-resident data set (--windows / --stride / --flip / --reverse / --shuffle / --data-seed / --balance /
    --label-shift; --align-report): every file is one segment, one data set serves all models of a --set, and the samples of an
    epoch are epoch_samples of the model's windows."""
    from .elements import Context

    where = a.eval_only or a.output
    jobs = set_jobs(a.records, where) if a.as_set else [(list(a.records), where)]
    mode, strides = a.windows or "skip", a.stride or (1,)
    files, val_files, rec_names = [], [], []
    for k, (fl, _) in enumerate(jobs):
        files.append([read_tfrecords(f, a.h_mb, a.w_mb) for f in fl])
        names = [] if not a.val else [f for f in a.val[k].split(",") if f] if a.as_set else list(a.val)
        val_files.append([read_tfrecords(f, a.h_mb, a.w_mb) for f in names])
        rec_names.append([f for f, (fr, _) in zip(list(fl) + names, files[k] + val_files[k]) if fr.shape[0]])
    capacity = sum(fr.shape[0] for group in files + val_files for fr, _ in group)
    if not capacity:
        raise ValueError("the records hold no frames")
    posts = post_settings(a, len(jobs))
    ctx = Context(a.device)
    data = TrainData(ctx, a.h_mb, a.w_mb, capacity)
    tables, val_tables = [], ([] if a.val or a.val_frac is not None else None)
    shifted = a.label_shift is not None or a.align_report is not None
    shifts = [] if a.label_shift is not None else None          # per model: the shift of every row of its table
    for k in range(len(jobs)):
        segs = [data.append(fr, gt) for fr, gt in files[k] if fr.shape[0]]
        vsegs = [data.append(fr, gt) for fr, gt in val_files[k] if fr.shape[0]]
        if a.record_report:
            _record_report(a, data, list(zip(rec_names[k], segs + vsegs)), k)
            continue
        if shifted:
            rec_shifts = _recording_shifts(a, data, list(zip(rec_names[k], segs + vsegs)), None if posts is None else posts[k].get("keep"))
            if rec_shifts is None:
                continue
        if a.val_frac is not None:
            segs, vsegs = split_frames_tail(segs, a.val_frac)
        if shifted:
            t, sh = _shifted_windows(segs, rec_shifts, mode, strides)
            tables.append(t)
            shifts.append(sh)
            if val_tables is not None:
                vt, vsh = _shifted_windows(vsegs, rec_shifts, mode, strides)
                val_tables.append(epoch_samples(vt, (min(strides),), label_shift=vsh))   # scored as they are, at their shift
        else:
            tables.append(windows(segs, mode, strides))
            if val_tables is not None:
                val_tables.append(windows(vsegs, mode, strides))
        print((f"model {k}: " if a.as_set else "") + f"{sum(b - s for s, b in segs)} frames -> {tables[k].shape[0]} windows of "
              f"{a.h_mb}x{a.w_mb}" + (f", {val_tables[k].shape[0]} to validate" if val_tables is not None else ""), file=sys.stderr)
    del files, val_files
    if a.align_report is not None or a.record_report:
        data.close()
        ctx.close()
        return 0
    if a.eval_only and shifts is not None:
        tables = [epoch_samples(t, (min(strides),), label_shift=sh) for t, sh in zip(tables, shifts)]
    if a.eval_only:
        ts = TrainerSet(ctx, a.h_mb, a.w_mb, weights=[_read_weights(p) for _, p in jobs], max_batch=a.batch)
        _apply_posts(ts, posts)
        ts.set_math(a.math)
        for k, ((_, path), ev) in enumerate(zip(jobs, ts.evaluate_data(data, tables, min(strides)))):
            if posts is not None:
                thr, keep = ts.get_post(k)
                ev["post"] = {"logit_thresh": thr, "ignored": int((keep == 0).sum())}
            print(json.dumps({"weights": path, **ev}))
    else:
        if a.as_set:
            os.makedirs(a.output, exist_ok=True)
            init = [_read_weights(p) for p in init_paths(a.records, a.init)] if a.init else None
        else:
            init = [_read_weights(a.init)] if a.init else None
        ts = TrainerSet(ctx, a.h_mb, a.w_mb, weights=init, n_models=len(jobs), seeds=[a.seed + k for k in range(len(jobs))],
                        max_batch=a.batch, **_plan_kw(a))
        ts._tag_models = a.as_set
        _apply_posts(ts, posts)
        ts.set_math(a.math)
        start = _resume(ts, a, len(jobs))
        ts.fit_data(data, tables, epochs=a.epochs, batch=a.batch, strides=strides, shuffle=a.shuffle, flip=a.flip or (),
                    reverse=a.reverse, data_seed=a.data_seed or 0, val_tables=val_tables, log=lambda s: print(s, file=sys.stderr),
                    keep=a.keep, checkpoint=a.checkpoint, start_epoch=start, balance=a.balance, label_shift=shifts)
        for k, (_, out) in enumerate(jobs):
            with open(out, "wb") as f:
                f.write(ts.best_weights_bytes(k) if a.keep == "best" else ts.weights_bytes(k))
    ts.close()
    data.close()
    ctx.close()
    return 0


def main(argv=None) -> int:
    a = parse_args(argv)
    if a.resident:
        return main_resident(a)
    if a.eval_only:
        return main_eval(a)
    if a.as_set:
        return main_set(a)
    from .elements import Context

    n_frames, records = _load(a.records, a)
    val = None
    if a.val:
        val = _load(a.val, a)[1]
    elif a.val_frac is not None:
        records, val = split_tail(*records, a.val_frac)
    print(f"{n_frames} frames -> {records[0].shape[0]} samples of {a.h_mb}x{a.w_mb}"
          + (f", {val[0].shape[0]} to validate" if val is not None else ""), file=sys.stderr)
    posts = post_settings(a, 1)
    ctx = Context(a.device)
    tr = Trainer(ctx, a.h_mb, a.w_mb, max_batch=a.batch, seed=a.seed, weights_flat=_read_weights(a.init) if a.init else None,
                 **_plan_kw(a))
    _apply_posts(tr, posts)
    tr.set_math(a.math)
    start = _resume(tr, a, 1)
    tr.fit(records, epochs=a.epochs, batch=a.batch, log=lambda s: print(s, file=sys.stderr), val=val, keep=a.keep,
           checkpoint=a.checkpoint, start_epoch=start)
    with open(a.output, "wb") as f:
        f.write(tr.best_weights_bytes() if a.keep == "best" else tr.weights_bytes())
    tr.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
