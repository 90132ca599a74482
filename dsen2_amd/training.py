"""Host side of fine-tuning (the counterpart of training/supres_train.py and the keras pieces it uses).

  Nadam              keras 2.2 Nadam: the per-step scalars, computed here in double; the update itself is the
                     dsen2_nadam_step kernel
  ReduceLROnPlateau  keras-2 logic (supres_train.py: factor 0.5, patience 5, min_delta 1e-6, cooldown 20, min_lr 1e-5)
  ModelCheckpoint    save_best_only on val_loss, written as a flat .npy that weights.load_flat reads
  History            what S2Model.fit returns
  AugmentOps         the per-sample flips and rotations of fit(augment=True) (not in the reference)
  load_training_data the reference's data layout (utils/patches.py: OpenDataFiles / splitTrainVal)
"""
import glob
import os

import numpy as np

SCALE = 2000


class Nadam(object):
    """keras.optimizers.Nadam(lr, beta_1, beta_2, epsilon, schedule_decay) as of keras 2.2.  `iterations` counts the steps
    taken; next_step() advances it and returns the scalars of that step (t 1-based, m_schedule starting at 1)."""

    def __init__(self, lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=1e-8, schedule_decay=0.004):
        self.lr = float(lr)
        self.beta_1 = float(beta_1)
        self.beta_2 = float(beta_2)
        self.epsilon = float(epsilon)
        self.schedule_decay = float(schedule_decay)
        self.iterations = 0
        self.m_schedule = 1.0

    def next_step(self):
        t = self.iterations + 1
        b1, sd = self.beta_1, self.schedule_decay
        mc_t = b1 * (1.0 - 0.5 * 0.96 ** (t * sd))
        mc_t1 = b1 * (1.0 - 0.5 * 0.96 ** ((t + 1) * sd))
        ms_new = self.m_schedule * mc_t
        ms_next = ms_new * mc_t1
        self.m_schedule = ms_new
        self.iterations = t
        return dict(t=t, lr=self.lr, b1=b1, b2=self.beta_2, eps=self.epsilon, mc_t=mc_t, mc_t1=mc_t1, ms_new=ms_new,
                    ms_next=ms_next, b2_pow_t=self.beta_2 ** t)

    def reset(self):
        """Fresh optimizer state (what keras has after compile(): --resume loads weights only)."""
        self.iterations = 0
        self.m_schedule = 1.0


class AugmentOps(object):
    """The flips and rotations of fit(augment=True): draw(n) returns the ops of the next step, one per sample of the (global)
    batch — int32 values uniform in 0..7, op = k + 4 f: f = 1 flips left-right first, then k quarter turns counter-clockwise
    (include/dsen2_hip.h, "dihedral").  The generator is numpy's default_rng on the seed sequence [seed, STREAM]: a function of
    the fit's seed alone, and a stream of its own — the epoch permutations (default_rng(seed)) are those of a fit without
    augmentation.  seed None: fresh entropy.  Every draw advances the stream, so equal seeds and equal batch sizes give equal
    ops, step for step, in any process."""
    STREAM = 0x64696865          # 'dihe'

    def __init__(self, seed=None):
        entropy = None if seed is None else [int(seed), self.STREAM]
        self.rng = np.random.default_rng(np.random.SeedSequence(entropy))

    def draw(self, n):
        return self.rng.integers(0, 8, size=int(n), dtype=np.int32)


class Callback(object):
    model = None

    def set_model(self, model):
        self.model = model

    def on_train_begin(self, logs=None):
        pass

    def on_epoch_end(self, epoch, logs=None):
        pass


class ReduceLROnPlateau(Callback):
    """keras 2.2 ReduceLROnPlateau, mode 'min' (val_loss).  step(current, lr) is the decision alone: the new learning rate."""

    def __init__(self, monitor='val_loss', factor=0.5, patience=5, verbose=0, min_delta=1e-6, cooldown=20, min_lr=1e-5):
        if factor >= 1.0:
            raise ValueError('ReduceLROnPlateau does not support a factor >= 1.0')
        self.monitor = monitor
        self.factor = float(factor)
        self.patience = int(patience)
        self.verbose = verbose
        self.min_delta = float(min_delta)
        self.cooldown = int(cooldown)
        self.min_lr = float(min_lr)
        self.on_train_begin()

    def on_train_begin(self, logs=None):
        self.best = np.inf
        self.wait = 0
        self.cooldown_counter = 0

    def in_cooldown(self):
        return self.cooldown_counter > 0

    def step(self, current, lr):
        if self.in_cooldown():
            self.cooldown_counter -= 1
            self.wait = 0
        if current < self.best - self.min_delta:
            self.best = current
            self.wait = 0
        elif not self.in_cooldown():
            self.wait += 1
            if self.wait >= self.patience and lr > self.min_lr:
                lr = max(lr * self.factor, self.min_lr)
                self.cooldown_counter = self.cooldown
                self.wait = 0
        return lr

    def on_epoch_end(self, epoch, logs=None):
        logs = logs if logs is not None else {}
        current = logs.get(self.monitor)
        if current is None:
            return
        old = self.model.optimizer.lr
        new = self.step(current, old)
        if new != old:
            self.model.optimizer.lr = new
            if self.verbose:
                print('\nEpoch %05d: ReduceLROnPlateau reducing learning rate to %s.' % (epoch + 1, new))


class ModelCheckpoint(Callback):
    """keras ModelCheckpoint(filepath, monitor='val_loss', save_best_only=True): the weights as a flat .npy."""

    def __init__(self, filepath, monitor='val_loss', verbose=0, save_best_only=True):
        self.filepath = filepath
        self.monitor = monitor
        self.verbose = verbose
        self.save_best_only = save_best_only
        self.best = np.inf

    def on_epoch_end(self, epoch, logs=None):
        logs = logs if logs is not None else {}
        current = logs.get(self.monitor)
        if self.save_best_only:
            if current is None or not current < self.best:
                return
            if self.verbose:
                print('\nEpoch %05d: %s improved from %.5f to %.5f, saving model to %s'
                      % (epoch + 1, self.monitor, self.best, current, self.filepath))
            self.best = current
        self.model.save_weights(self.filepath)


class History(object):
    def __init__(self):
        self.epoch = []
        self.history = {}

    def append(self, epoch, logs):
        self.epoch.append(epoch)
        for k, v in logs.items():
            self.history.setdefault(k, []).append(v)


class MaskedTarget(np.ndarray):
    """A target array cut from a corpus whose ground truth carries a class mask as no-data (corpus.TileCorpus(class_masks=)): an
    ndarray like any other, which fit recognises (check_masked_target).  Views and slices keep the type."""
    class_masked = True


def check_masked_target(setting, masked, who):
    """ValueError when a target that carries a class mask (`masked`) meets a loss setting without the no-data mask: the masked
    pixels are zeros in the ground truth, and a loss that does not ignore them would train the network towards zeros."""
    from . import losses
    if masked and losses.pointwise(setting)[2] != losses.MASK_NODATA:
        raise ValueError('%s: the ground truth carries a class mask as no-data, but the model was not compiled with mask_nodata=True: '
                         'a mask that the loss ignores would train on zeros' % who)


def load_training_data(path, run_60=False, scale=SCALE):
    """utils/patches.py OpenDataFiles + splitTrainVal: every <path>/train/*SAFE (train60/ for run_60) directory's data10,
    data20 (, data60) and ground truth data20_gt (data60_gt) arrays, concatenated in sorted directory order, divided by
    `scale`, and split by the boolean mask <train dir>/val_index.npy.  Returns (train, label, val_tr, val_lb) with
    train / val_tr lists of NCHW float32 arrays."""
    train_path = os.path.join(path, 'train60' if run_60 else 'train')
    dirs = sorted(glob.glob(os.path.join(train_path, '*SAFE')))
    if not dirs:
        raise OSError('no *SAFE directories under %s' % train_path)
    names = ['data10', 'data20'] + (['data60'] if run_60 else [])
    gt = 'data60_gt' if run_60 else 'data20_gt'
    parts = {k: [] for k in names + [gt]}
    for d in dirs:
        for k in parts:
            parts[k].append(np.load(os.path.join(d, k + '.npy')))
    arrays = {k: np.concatenate(v).astype(np.float32) for k, v in parts.items()}
    if scale:
        for k in arrays:
            arrays[k] /= np.float32(scale)
    val_ind = np.load(os.path.join(train_path, 'val_index.npy')).astype(bool)
    train = [arrays[k][~val_ind] for k in names]
    val_tr = [arrays[k][val_ind] for k in names]
    return train, arrays[gt][~val_ind], val_tr, arrays[gt][val_ind]
