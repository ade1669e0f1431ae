"""Training sets without a GPU: argument checks of the covahip_train_*_set / _m entry points, the step plan of
TrainerSet.fit, and the --set command line."""
import ctypes as C
import os

import numpy as np
import pytest

from cova_amd import _lib as L, train as T, weights as W

INVALID = 1


def test_set_entry_points_refuse_null_and_out_of_range_without_a_device():
    lib = L.lib()
    cfg = L.TrainCfg()
    lib.covahip_train_default_cfg(C.byref(cfg))
    blob = W.to_bytes(np.zeros(W.N_PARAMS, np.float32))
    ptrs = (C.c_char_p * 2)(blob, blob)
    sizes = (C.c_size_t * 2)(len(blob), len(blob))
    seeds = (C.c_uint64 * 2)(1, 2)
    h = C.c_void_p(1234)
    fake = C.c_void_p(8)   # never dereferenced: every call below fails its argument checks first
    assert lib.covahip_train_create_set(None, C.byref(cfg), 2, ptrs, sizes, seeds, C.byref(h)) == INVALID
    assert not h.value     # *out is cleared on failure
    assert lib.covahip_train_create_set(fake, None, 2, ptrs, sizes, seeds, C.byref(h)) == INVALID
    assert lib.covahip_train_create_set(fake, C.byref(cfg), 2, None, sizes, seeds, C.byref(h)) == INVALID
    assert lib.covahip_train_create_set(fake, C.byref(cfg), 2, ptrs, None, seeds, C.byref(h)) == INVALID
    assert lib.covahip_train_create_set(fake, C.byref(cfg), 2, ptrs, sizes, seeds, None) == INVALID
    for n in (0, -1, 257):
        assert lib.covahip_train_create_set(fake, C.byref(cfg), n, ptrs, sizes, seeds, C.byref(h)) == INVALID, n
    holes = (C.c_char_p * 2)(blob, None)
    assert lib.covahip_train_create_set(fake, C.byref(cfg), 2, holes, sizes, None, C.byref(h)) == INVALID
    bad = L.TrainCfg.from_buffer_copy(cfg)
    bad.max_batch = 0
    assert lib.covahip_train_create_set(fake, C.byref(bad), 2, ptrs, sizes, seeds, C.byref(h)) == INVALID
    # a malformed blob in any slot is refused before the device is touched
    short = (C.c_size_t * 2)(len(blob), len(blob) - 4)
    assert lib.covahip_train_create_set(fake, C.byref(cfg), 2, ptrs, short, seeds, C.byref(h)) == 6   # COVAHIP_ERR_BAD_WEIGHTS
    n = C.c_int()
    assert lib.covahip_train_num_models(None, C.byref(n)) == INVALID
    b = (C.c_int32 * 2)(1, 1)
    f = (C.c_float * 2)(1e-3, 1e-3)
    x = np.zeros(16, np.uint8)
    assert lib.covahip_train_step_set(None, x.ctypes.data, x.ctypes.data, b, f, f, L.MEM_HOST) == INVALID
    v = (C.c_int64 * 3)()
    sz = C.c_size_t()
    assert lib.covahip_train_metrics_m(None, 0, v) == INVALID
    assert lib.covahip_train_weights_m(None, 0, None, 0, C.byref(sz)) == INVALID
    assert lib.covahip_train_grads_m(None, 0, x.ctypes.data, W.N_PARAMS) == INVALID


def _walk(plan, k):
    return [st[k] for st in plan]


def test_epoch_plan_unequal_sizes():
    plan = T.set_epoch_plan([10, 4, 7], 4)
    assert len(plan) == 3 and all(len(st) == 3 for st in plan)
    assert _walk(plan, 0) == [(0, 4), (4, 4), (8, 2)]
    assert _walk(plan, 1) == [(0, 4), (4, 0), (4, 0)]         # batch 0 once its epoch is over
    assert _walk(plan, 2) == [(0, 4), (4, 3), (7, 0)]
    for k, size in enumerate([10, 4, 7]):
        seen = [i for a, n in _walk(plan, k) for i in range(a, a + n)]
        assert seen == list(range(size))                       # every sample once, in order
        counts = [n for _, n in _walk(plan, k)]
        solo = [min(4, size - i) for i in range(0, size, 4)]   # Trainer.fit's batches
        assert counts[:len(solo)] == solo and not any(counts[len(solo):])
    assert all(any(n for _, n in st) for st in plan)           # no step with every batch 0


@pytest.mark.parametrize("sizes,batch", [([1], 4), ([4, 4], 4), ([5, 1, 9, 8], 4), ([3, 17], 1), ([2, 3], 8)])
def test_epoch_plan_properties(sizes, batch):
    plan = T.set_epoch_plan(sizes, batch)
    assert len(plan) == max(-(-s // batch) for s in sizes)
    for k, size in enumerate(sizes):
        assert [i for a, n in _walk(plan, k) for i in range(a, a + n)] == list(range(size))
        assert all(0 <= n <= batch for _, n in _walk(plan, k))


def test_epoch_plan_refuses_empty():
    with pytest.raises(ValueError):
        T.set_epoch_plan([4, 0], 4)
    with pytest.raises(ValueError):
        T.set_epoch_plan([], 4)
    with pytest.raises(ValueError):
        T.set_epoch_plan([4], 0)


def test_set_command_line_and_output_names():
    a = T.parse_args(["--set", "-o", "out", "--seed", "5", "a/cam0.tfrecord", "cam1.tfrecord", "x/cam2a.tfrecord,cam2b.tfrecord"])
    assert a.as_set and a.output == "out" and a.seed == 5 and (a.batch, a.epochs, a.h_mb, a.w_mb) == (4, 20, 45, 80)
    jobs = T.set_jobs(a.records, a.output)
    assert [files for files, _ in jobs] == [["a/cam0.tfrecord"], ["cam1.tfrecord"], ["x/cam2a.tfrecord", "cam2b.tfrecord"]]
    assert [out for _, out in jobs] == [os.path.join("out", n) for n in ("cam0.cvhw", "cam1.cvhw", "cam2a.cvhw")]
    with pytest.raises(ValueError):
        T.set_jobs(["a/cam.tfrecord", "b/cam.tfrecord"], "out")          # two models, one file name
    with pytest.raises(ValueError):
        T.set_jobs(["cam.tfrecord", ","], "out")
    solo = T.parse_args(["r0.tfrecord", "r1.tfrecord", "-o", "w.cvhw"])   # without --set: as before
    assert not solo.as_set and solo.records == ["r0.tfrecord", "r1.tfrecord"] and solo.output == "w.cvhw"


def test_trainer_set_argument_checks():
    class NoCtx:
        handle = None

    with pytest.raises(ValueError):
        T.TrainerSet(NoCtx())                                              # neither weights nor n_models
    with pytest.raises(ValueError):
        T.TrainerSet(NoCtx(), weights=[T.init_weights(0)], n_models=2)
    with pytest.raises(ValueError):
        T.TrainerSet(NoCtx(), weights=[T.init_weights(0)], seeds=[1, 2])
    with pytest.raises(L.CovahipError) as e:
        T.TrainerSet(NoCtx(), 45, 80, weights=[T.init_weights(0)])         # a null ctx is refused by the library
    assert e.value.status == 1
