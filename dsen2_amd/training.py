"""Host side of fine-tuning (the counterpart of training/supres_train.py and the keras pieces it uses).

  Nadam              keras 2.2 Nadam: the per-step scalars, computed here in double; the update itself is the
                     dsen2_nadam_step kernel
  Adam, SGD          keras 2.2's (no amsgrad, no decay=); with Nadam they share the keyword-only options clipnorm, clipvalue,
                     weight_decay, decay_bias (not in the reference): the step is then dsen2_optimizer_step
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


MAX_DECAY_RANGES = 128      # include/dsen2_hip.h, dsen2_optimizer_step


def decay_ranges(cin, cout, num_layers, feature_size, decay_bias=False):
    """The half-open index ranges of the keras-flat vector that decoupled weight decay applies to: every convolution kernel and
    no bias (weights.layer_shapes: kernel, then bias, layer by layer); decay_bias=True: the whole vector as one range."""
    from . import weights
    shapes = weights.layer_shapes(cin, cout, num_layers, feature_size)
    if decay_bias:
        return [(0, weights.num_params(cin, cout, num_layers, feature_size))]
    out, off = [], 0
    for ci, co in shapes:
        out.append((off, off + 9 * ci * co))
        off += 9 * ci * co + co
    if len(out) > MAX_DECAY_RANGES:
        raise ValueError('weight decay takes at most %d ranges; this network has %d kernels' % (MAX_DECAY_RANGES, len(out)))
    return out


class Optimizer(object):
    """What Nadam, Adam and SGD share: the step counter, a mutable `.lr` (ReduceLROnPlateau writes it) and the keyword-only options
    of the step (include/dsen2_hip.h, dsen2_optimizer_step).  clipnorm > 0: the gradient is scaled by clipnorm / n where its
    global norm n over ALL weight tensors is >= clipnorm (keras 2.2 get_gradients); clipvalue > 0: every element is then clamped to
    [-clipvalue, clipvalue]; weight_decay > 0: decoupled decay (AdamW's), p -= lr * weight_decay * p_old after the update, on the
    convolution kernels, and on the biases too with decay_bias=True.  0 switches an option off.  The options are plain
    attributes like lr: a step follows them as they stand when it is taken."""
    KIND = None

    def _init_options(self, lr, clipnorm, clipvalue, weight_decay, decay_bias):
        self.lr = float(lr)
        for name, x in (('clipnorm', clipnorm), ('clipvalue', clipvalue), ('weight_decay', weight_decay)):
            x = float(x)
            if not 0.0 <= x < float('inf'):
                raise ValueError('%s must be finite and >= 0, got %r' % (name, x))
            setattr(self, name, x)
        self.decay_bias = bool(decay_bias)
        self.iterations = 0

    def has_options(self):
        return bool(self.clipnorm or self.clipvalue or self.weight_decay)

    def step_state(self):
        """What next_step() changes, for taking a refused step back."""
        return (self.iterations,)

    def set_step_state(self, state):
        (self.iterations,) = state

    def reset(self):
        """Fresh optimizer state (what keras has after compile(): --resume loads weights only)."""
        self.iterations = 0


class Nadam(Optimizer):
    """keras.optimizers.Nadam(lr, beta_1, beta_2, epsilon, schedule_decay) as of keras 2.2.  `iterations` counts the steps
    taken; next_step() advances it and returns the scalars of that step (t 1-based, m_schedule starting at 1).  The keyword-only
    options are Optimizer's; without them the step is the dsen2_nadam_step kernel, as it always was."""
    KIND = 0

    def __init__(self, lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=1e-8, schedule_decay=0.004, *, clipnorm=0.0, clipvalue=0.0,
                 weight_decay=0.0, decay_bias=False):
        self._init_options(lr, clipnorm, clipvalue, weight_decay, decay_bias)
        self.beta_1 = float(beta_1)
        self.beta_2 = float(beta_2)
        self.epsilon = float(epsilon)
        self.schedule_decay = float(schedule_decay)
        self.m_schedule = 1.0

    def step_state(self):
        return (self.iterations, self.m_schedule)

    def set_step_state(self, state):
        self.iterations, self.m_schedule = state

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


class Adam(Optimizer):
    """keras.optimizers.Adam(lr, beta_1, beta_2, epsilon) as of keras 2.2, without amsgrad and without `decay`.  next_step()
    returns the scalars of step t (1-based): lr_t = lr * sqrt(1 - beta_2^t) / (1 - beta_1^t), in double."""
    KIND = 1

    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-8, *, clipnorm=0.0, clipvalue=0.0, weight_decay=0.0,
                 decay_bias=False):
        self._init_options(lr, clipnorm, clipvalue, weight_decay, decay_bias)
        self.beta_1 = float(beta_1)
        self.beta_2 = float(beta_2)
        self.epsilon = float(epsilon)

    def next_step(self):
        t = self.iterations + 1
        self.iterations = t
        lr_t = self.lr * np.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t)
        return dict(t=t, lr=self.lr, b1=self.beta_1, b2=self.beta_2, eps=self.epsilon, lr_t=float(lr_t))


class SGD(Optimizer):
    """keras.optimizers.SGD(lr, momentum, nesterov) as of keras 2.2, without `decay`: velocity = momentum * velocity - lr * g;
    p += velocity, or with nesterov=True p += momentum * velocity - lr * g."""
    KIND = 2

    def __init__(self, lr=0.01, momentum=0.0, nesterov=False, *, clipnorm=0.0, clipvalue=0.0, weight_decay=0.0, decay_bias=False):
        self._init_options(lr, clipnorm, clipvalue, weight_decay, decay_bias)
        self.momentum = float(momentum)
        if not 0.0 <= self.momentum < 1.0:
            raise ValueError('momentum must be in [0, 1), got %r' % self.momentum)
        self.nesterov = bool(nesterov)

    def next_step(self):
        self.iterations += 1
        return dict(t=self.iterations, lr=self.lr, momentum=self.momentum, nesterov=self.nesterov)


OPTIMIZERS = {'nadam': Nadam, 'adam': Adam, 'sgd': SGD}


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
