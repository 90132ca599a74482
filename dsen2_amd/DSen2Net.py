"""Host-side mirror of the reference's network module (utils/DSen2Net.py) over libdsen2_hip.so.

``s2model(input_shape, num_layers, feature_size)`` keeps the reference's name, arguments and defaults
(utils/DSen2Net.py:18) and returns an object with the two keras.Model methods the inference path uses:
``load_weights(path)`` (testing/supres.py:63) and ``predict(list_of_arrays, verbose=...)`` (supres.py:65).
All arithmetic happens in the HIP kernels behind the C ABI; PyTorch-ROCm only provides device buffers,
H2D/D2H copies and the stream.
"""
import ctypes
import sys
import threading

import numpy as np
import torch

from . import _lib, weights as _weights

RES_SCALE = 0.1   # resBlock(scale=0.1), utils/DSen2Net.py:9
# arithmetic of the residual-block convolutions (include/dsen2_hip.h: dsen2_model_create).  'fp32' is what keras computes and
# the default everywhere; 'bf16' = bf16 operands (~1e-3 relative error); 'bf16x3' = every fp32 operand as two bf16 numbers,
# three bf16 MFMAs per product (~1e-5 whole-network rmse, inside the 1e-4 gate; ~3 x the fp32 rate)
PRECISIONS = {'fp32': 0, 'bf16': 1, 'bf16x3': 2}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# -- the 8 flips and rotations of a patch (include/dsen2_hip.h, "dihedral") ------------------------------------------------------
# op = k + 4 f: D_op(a) = np.rot90(a[..., ::-1] if f else a, k, axes=(-2, -1)); odd k swaps H and W.
def ensemble_mask(ensemble):
    """The 8-bit member mask of dsen2_model_forward_ensemble: False / None -> 0 (no ensemble), True -> 255 (all 8 members), an
    iterable of ops 0..7 -> their bits."""
    if ensemble is None or ensemble is False:
        return 0
    if ensemble is True:
        return 255
    mask = 0
    for op in ensemble:
        if int(op) != op or not 0 <= int(op) <= 7:
            raise ValueError('an ensemble member must be an op 0..7, got %r' % (op,))
        mask |= 1 << int(op)
    if mask == 0:
        raise ValueError('an ensemble needs at least one member')
    return mask


def dihedral(x, op=None, ops=None, inverse=False, out=None):
    """D_op(x), or D_op^-1(x) when `inverse`, of a contiguous float32 CUDA tensor [n, c, h, w] (dsen2_dihedral_nchw): one op for
    the whole tensor (`op`, 0..7), or one per sample (`ops`: n values 0..7, a sequence or an int32 CUDA tensor; square images
    only).  Returns `out` (allocated when None): [n, c, w, h] for odd op & 3."""
    if not torch.cuda.is_available():
        raise RuntimeError('dsen2_amd needs a ROCm GPU (gfx950); there is no CPU fallback')
    if (op is None) == (ops is None):
        raise ValueError('give either op (one for the tensor) or ops (one per sample)')
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
        raise ValueError('x must be a contiguous float32 CUDA tensor [n, c, h, w], got %r %s %s' % (tuple(x.shape), x.dtype, x.device))
    n, c, h, w = x.shape
    ops_dev = None
    if ops is not None:
        if h != w:
            raise ValueError('per-sample ops need square images (an odd rotation swaps H and W), got %dx%d' % (h, w))
        if isinstance(ops, torch.Tensor):
            ops_dev = ops
        else:
            host = np.ascontiguousarray(ops, dtype=np.int32)
            if host.size and (host.min() < 0 or host.max() > 7):
                raise ValueError('ops must be 0..7, got %r' % (host.tolist(),))
            ops_dev = torch.from_numpy(host).to(x.device)
        if tuple(ops_dev.shape) != (n,) or ops_dev.dtype != torch.int32 or not ops_dev.is_contiguous() or ops_dev.device != x.device:
            raise ValueError('ops must hold one int32 per sample (%d) on %s' % (n, x.device))
        op = 0
    elif int(op) != op or not 0 <= int(op) <= 7:
        raise ValueError('op must be 0..7, got %r' % (op,))
    shape = (n, c, w, h) if int(op) & 1 else (n, c, h, w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError('out must be a contiguous float32 %s tensor of shape %r, got %r %s' % (x.device, shape, tuple(out.shape), out.dtype))
    with torch.cuda.device(x.device):
        _lib.call('dsen2_dihedral_nchw', _ptr(x), _ptr(out), n, c, h, w, int(op), _ptr(ops_dev), int(bool(inverse)),
                  _stream_ptr(x.device))
    return out


class S2Model(object):
    """What keras' Model is to the reference: built by s2model(), then load_weights() and predict()."""

    def __init__(self, input_shape, num_layers, feature_size, device=None, precision='fp32'):
        if len(input_shape) not in (2, 3):
            raise ValueError('input_shape must describe 2 or 3 inputs, got %r' % (input_shape,))
        if not torch.cuda.is_available():
            raise RuntimeError('dsen2_amd needs a ROCm GPU (gfx950); there is no CPU fallback')
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.bands = tuple(int(s[0]) for s in input_shape)
        self.num_layers = int(num_layers)
        self.feature_size = int(feature_size)
        self.cin = sum(self.bands)
        self.cout = self.bands[-1]          # utils/DSen2Net.py:35 — input_shape[-1][0]
        self._handle = ctypes.c_void_p(0)
        c60 = self.bands[2] if len(self.bands) == 3 else 0
        with torch.cuda.device(self.device):
            if precision not in PRECISIONS:
                raise ValueError("precision must be one of %s" % ', '.join(repr(k) for k in PRECISIONS))
            self.precision = precision
            _lib.call('dsen2_model_create', ctypes.byref(self._handle), self.bands[0], self.bands[1], c60,
                      self.num_layers, self.feature_size, PRECISIONS[precision])
        # One workspace per STREAM the model is used from (keyed by the stream's handle): SURVEY §8(b) — "calls on a
        # handle are serialised by the given stream" — so forwards enqueued on different streams, from one thread or
        # several, must not share the activation buffers the kernels of both would be writing.
        self._workspaces = {}
        self._ws_lock = threading.Lock()
        self.max_workspace_bytes = 6 << 30   # predict() and the tile path size their batches to stay below this
        self.optimizer = None                # compile() (training)
        self._train = None                   # device weights, gradient and optimizer state of a compiled model
        self._error_work = None              # scratch of abs_sq_error_sums_device (used on the training stream alone)

    # -- keras.Model surface -------------------------------------------------------------------
    def count_params(self):
        return int(_lib.load().dsen2_model_num_params(self._handle))

    def set_weights_flat(self, flat):
        flat = np.ascontiguousarray(flat, np.float32).ravel()
        with torch.cuda.device(self.device):
            _lib.call('dsen2_model_load_weights', self._handle,
                      flat.ctypes.data_as(_lib.c_float_p), flat.size)
            if self._train is not None:      # a model being trained continues from the new weights
                self._train['flat'].copy_(torch.from_numpy(flat))

    def load_weights(self, path):
        self.set_weights_flat(_weights.load_flat(path, self.cin, self.cout, self.num_layers, self.feature_size))

    def workspace_bytes(self, n, h, w, ensemble=False):
        """Scratch of one forward of n patches of h x w; ensemble (True, or the member ops): of the self-ensemble forward, which
        also holds the turned inputs and one member's output."""
        out = ctypes.c_size_t(0)
        mask = ensemble_mask(ensemble)
        if mask:
            _lib.call('dsen2_model_ensemble_workspace_bytes', self._handle, n, h, w, mask, ctypes.byref(out))
        else:
            _lib.call('dsen2_model_workspace_bytes', self._handle, n, h, w, ctypes.byref(out))
        return out.value

    def _get_workspace(self, nbytes):
        """The current stream's workspace, grown on demand.  Allocated under that stream, so torch's caching allocator
        hands a replaced (smaller) buffer back only to work ordered after the kernels still reading it."""
        key = torch.cuda.current_stream(self.device).cuda_stream
        with self._ws_lock:
            ws = self._workspaces.get(key)
            if ws is None or ws.numel() < nbytes:
                self._workspaces.pop(key, None)
                ws = None
                ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                self._workspaces[key] = ws
            return ws

    def release_workspaces(self):
        """Drop every stream's activation buffers (they are re-created on the next forward)."""
        with self._ws_lock:
            self._workspaces.clear()

    def forward_device(self, xs, out=None):
        """One batch entirely on the device: xs = list of contiguous float32 CUDA tensors [n,c,h,w]."""
        if len(xs) != len(self.bands):
            raise ValueError('expected %d inputs, got %d' % (len(self.bands), len(xs)))
        n, _, h, w = xs[0].shape
        for x, c in zip(xs, self.bands):
            if tuple(x.shape) != (n, c, h, w) or x.dtype != torch.float32 or not x.is_contiguous() or \
                    x.device != self.device:
                raise ValueError('input must be a contiguous float32 %s tensor of shape %r, got %r %s %s'
                                 % (self.device, (n, c, h, w), tuple(x.shape), x.dtype, x.device))
        out = self._check_out(out, n, h, w)
        if n == 0:
            return out
        ws = self._get_workspace(self.workspace_bytes(n, h, w))
        with torch.cuda.device(self.device):
            _lib.call('dsen2_model_forward', self._handle, _ptr(xs[0]), _ptr(xs[1]),
                      _ptr(xs[2]) if len(xs) == 3 else ctypes.c_void_p(0), _ptr(out), n, h, w,
                      _ptr(ws), ws.numel(), _stream_ptr(self.device))
        return out

    def forward_device_ensemble(self, xs, out=None, ops=range(8)):
        """The geometric self-ensemble of one batch on the device (dsen2_model_forward_ensemble): the mean over the member ops
        (default all 8) of D_op^-1(forward(D_op xs)), members in ascending op order, summed in fp32, then divided by their number.
        ops=[0] is forward_device bit for bit.  xs and out as forward_device."""
        ops = list(range(8)) if ops is True else list(ops)
        mask = ensemble_mask(ops)
        if len(xs) != len(self.bands):
            raise ValueError('expected %d inputs, got %d' % (len(self.bands), len(xs)))
        n, _, h, w = xs[0].shape
        for x, c in zip(xs, self.bands):
            if tuple(x.shape) != (n, c, h, w) or x.dtype != torch.float32 or not x.is_contiguous() or \
                    x.device != self.device:
                raise ValueError('input must be a contiguous float32 %s tensor of shape %r, got %r %s %s'
                                 % (self.device, (n, c, h, w), tuple(x.shape), x.dtype, x.device))
        out = self._check_out(out, n, h, w)
        if n == 0:
            return out
        ws = self._get_workspace(self.workspace_bytes(n, h, w, ensemble=ops))
        with torch.cuda.device(self.device):
            _lib.call('dsen2_model_forward_ensemble', self._handle, _ptr(xs[0]), _ptr(xs[1]),
                      _ptr(xs[2]) if len(xs) == 3 else ctypes.c_void_p(0), _ptr(out), n, h, w, mask,
                      _ptr(ws), ws.numel(), _stream_ptr(self.device))
        return out

    def _check_out(self, out, n, h, w):
        """The raw pointer of `out` goes straight to the kernels: a wrong-sized, strided or other-device tensor
        would be written out of bounds or in the wrong place."""
        if out is None:
            return torch.empty((n, self.cout, h, w), dtype=torch.float32, device=self.device)
        if tuple(out.shape) != (n, self.cout, h, w) or out.dtype != torch.float32 or not out.is_contiguous() or \
                out.device != self.device:
            raise ValueError('out must be a contiguous float32 %s tensor of shape %r, got %r %s %s (contiguous: %s)'
                             % (self.device, (n, self.cout, h, w), tuple(out.shape), out.dtype, out.device,
                                out.is_contiguous()))
        return out

    def time_body_in_forward(self, xs, out=None, iters=10):
        """Mean duration (ms) of ONE residual-block convolution launch inside `iters` full forward passes on `xs`
        (HIP events on the launch stream around the 2*num_layers body convolutions of each pass): the duration the
        kernel has in the running network — bench.py's roofline measurement."""
        n, _, h, w = xs[0].shape
        out = self._check_out(out, n, h, w)
        ws = self._get_workspace(self.workspace_bytes(n, h, w))
        ms = ctypes.c_float(0)
        with torch.cuda.device(self.device):
            _lib.call('dsen2_model_forward_timed', self._handle, _ptr(xs[0]), _ptr(xs[1]),
                      _ptr(xs[2]) if len(xs) == 3 else ctypes.c_void_p(0), _ptr(out), n, h, w,
                      _ptr(ws), ws.numel(), _stream_ptr(self.device), int(iters), ctypes.byref(ms))
        return ms.value

    def profile_forward(self, xs, out=None, iters=10, warm=3):
        """`warm` plain forward passes, then — the stream never idling in between — `iters` passes on `xs` with four HIP
        events each (dsen2_model_forward_profile).  Mean milliseconds: forward_ms (first event to last of a pass), first_ms /
        body_ms / out_ms (first convolution, all 2*num_layers residual-block convolutions, output convolution: consecutive
        intervals, they add up to forward_ms) and wall_ms (per instrumented pass, first event of the first pass to last event
        of the last: a pass with its event records and the gap to the next one)."""
        n, _, h, w = xs[0].shape
        out = self._check_out(out, n, h, w)
        ws = self._get_workspace(self.workspace_bytes(n, h, w))
        ms = (ctypes.c_float * 5)()
        with torch.cuda.device(self.device):
            _lib.call('dsen2_model_forward_profile', self._handle, _ptr(xs[0]), _ptr(xs[1]),
                      _ptr(xs[2]) if len(xs) == 3 else ctypes.c_void_p(0), _ptr(out), n, h, w,
                      _ptr(ws), ws.numel(), _stream_ptr(self.device), int(warm), int(iters), ms)
        return dict(forward_ms=ms[0], first_ms=ms[1], body_ms=ms[2], out_ms=ms[3], wall_ms=ms[4])

    def body_launches(self, n, h, w):
        """Kernel launches the 2*num_layers residual-block convolutions of a batch take: 1 = one chain launch."""
        with torch.cuda.device(self.device):
            r = _lib.load().dsen2_model_body_launches(self._handle, int(n), int(h), int(w))
        if r < 0:
            raise _lib.DSen2Error(r, _lib.load().dsen2_last_error().decode())
        return r

    def batch_limit(self, h, w, ensemble=False):
        per = self.workspace_bytes(1, h, w, ensemble=ensemble)
        return max(1, int(self.max_workspace_bytes // per))

    def preferred_batch(self, h, w, ensemble=False):
        """The batch the tile path and predict() cut their work into: batch_limit() for fp32 and for large patches; in the
        bf16 modes, for patches the chain kernel takes (up to 64 x 64: there it is 1-3 % ahead of the per-layer launches and
        bit-identical to them; profiles/r04_k_chain_vs_layerwise.txt), the largest batch below the limit that runs ALL
        residual-block convolutions in one chain launch (body_launches() == 1: a multiple of the CU count).  Results never
        depend on the batch size.  ensemble (True, or the member ops): the same under the self-ensemble's larger workspace, the
        chain launch asked of the turned orientation as well."""
        # (off: the two-argument call, as before — a stand-in for batch_limit need not know the keyword)
        limit = self.batch_limit(h, w, ensemble=ensemble) if ensemble_mask(ensemble) else self.batch_limit(h, w)
        if self.precision == 'fp32' or self.num_layers <= 0:
            return limit
        turned = h != w and ensemble_mask(ensemble) & 0xAA       # an odd rotation among the members: w x h forwards too
        cus = int(torch.cuda.get_device_properties(self.device).multi_processor_count)
        n = (limit // cus) * cus
        while n >= cus:
            if self.body_launches(n, h, w) == 1 and (not turned or self.body_launches(n, w, h) == 1):
                return n
            n -= cus
        return limit

    def predict(self, x, batch_size=None, verbose=0, ensemble=False):
        """keras Model.predict: list of NCHW float32 ndarrays -> ndarray [N, cout, H, W].

        ``ensemble`` (not in keras; default off): True, or an iterable of ops 0..7 — every batch goes through
        forward_device_ensemble, the geometric self-ensemble over those members (True: all 8), at about as many times the cost.

        ``batch_size`` only bounds device memory (results do not depend on it); default: as many
        patches as fit ``max_workspace_bytes``.  Host<->device copies go through page-locked buffers on their own
        streams; with more than one batch, batch i+1 is staged and batch i-1 downloaded while batch i computes.
        Activation buffers are per stream: a model may be used from several streams / threads at once (the weights
        are read-only after load_weights).
        """
        xs = [np.ascontiguousarray(a, dtype=np.float32) for a in x]
        if len(xs) != len(self.bands):
            raise ValueError('expected %d inputs, got %d' % (len(self.bands), len(xs)))
        n, _, h, w = xs[0].shape
        for a, c in zip(xs, self.bands):
            if a.shape != (n, c, h, w):
                raise ValueError('input of shape %r where %r is expected' % (a.shape, (n, c, h, w)))
        mask = ensemble_mask(ensemble if isinstance(ensemble, bool) or ensemble is None else list(ensemble))
        members = [op for op in range(8) if (mask >> op) & 1]
        if batch_size is not None:
            bs = int(batch_size)
        else:
            bs = self.preferred_batch(h, w, ensemble=members) if members else self.preferred_batch(h, w)
        out = np.empty((n, self.cout, h, w), np.float32)
        if n == 0:
            return self._progress_end(verbose, out)
        starts = list(range(0, n, bs))
        bs = min(bs, n)
        with torch.cuda.device(self.device):
            comp = torch.cuda.current_stream(self.device)
            h2d, d2h = torch.cuda.Stream(self.device), torch.cuda.Stream(self.device)
            # one slot for a single batch, two to overlap staging / compute / download of consecutive batches; every
            # transfer goes through page-locked memory on its own stream (a pageable copy blocks the host and runs at
            # a fifth of the PCIe rate)
            slots = []
            for _ in range(min(2, len(starts))):
                slots.append(dict(
                    pin_in=[torch.empty((bs, c, h, w), dtype=torch.float32, pin_memory=True) for c in self.bands],
                    dev_in=[torch.empty((bs, c, h, w), dtype=torch.float32, device=self.device) for c in self.bands],
                    dev_out=torch.empty((bs, self.cout, h, w), dtype=torch.float32, device=self.device),
                    pin_out=torch.empty((bs, self.cout, h, w), dtype=torch.float32, pin_memory=True),
                    ev_in=torch.cuda.Event(), ev_comp=torch.cuda.Event(), ev_out=torch.cuda.Event(), span=None))

            def collect(slot):                      # batch whose download was issued from this slot
                if slot['span'] is not None:
                    slot['ev_out'].synchronize()
                    j0, j1 = slot['span']
                    out[j0:j1] = slot['pin_out'][:j1 - j0].numpy()
                    slot['span'] = None
                    self._progress(verbose, j1, n)

            for i, i0 in enumerate(starts):
                i1 = min(n, i0 + bs)
                m = i1 - i0
                slot = slots[i % len(slots)]
                collect(slot)                       # batch i-2: after this the slot's buffers are all free
                for k, a in enumerate(xs):          # host copy into page-locked memory, under batch i-1's compute
                    slot['pin_in'][k][:m].numpy()[...] = a[i0:i1]
                with torch.cuda.stream(h2d):
                    for k in range(len(xs)):
                        slot['dev_in'][k][:m].copy_(slot['pin_in'][k][:m], non_blocking=True)
                    slot['ev_in'].record(h2d)
                comp.wait_event(slot['ev_in'])
                if members:
                    self.forward_device_ensemble([t[:m] for t in slot['dev_in']], out=slot['dev_out'][:m], ops=members)
                else:
                    self.forward_device([t[:m] for t in slot['dev_in']], out=slot['dev_out'][:m])
                slot['ev_comp'].record(comp)
                with torch.cuda.stream(d2h):
                    d2h.wait_event(slot['ev_comp'])
                    slot['pin_out'][:m].copy_(slot['dev_out'][:m], non_blocking=True)
                    slot['ev_out'].record(d2h)
                slot['span'] = (i0, i1)
            last = len(starts) - 1
            if len(slots) > 1:
                collect(slots[(last - 1) % 2])
            collect(slots[last % len(slots)])
        return self._progress_end(verbose, out)

    @staticmethod
    def _progress(verbose, done, total):
        if verbose:
            sys.stdout.write('\r%d/%d' % (done, total))
            sys.stdout.flush()

    @staticmethod
    def _progress_end(verbose, out):
        if verbose:
            sys.stdout.write('\n')
        return out

    def time_body_conv(self, layer, x_in, aux, out, iters=10):
        """Mean duration (ms) of `iters` launches of body convolution `layer` (1-based), HIP events on the
        launch stream — bench.py's roofline measurement."""
        n, h, w, _ = x_in.shape
        ms = ctypes.c_float(0)
        with torch.cuda.device(self.device):
            _lib.call('dsen2_model_time_body_conv', self._handle, layer, _ptr(x_in), _ptr(aux), _ptr(out), n, h, w,
                      iters, _stream_ptr(self.device), ctypes.byref(ms))
        return ms.value

    # -- training (fp32 and bf16x3 models, fp32 ones optionally on bf16 operands; include/dsen2_hip.h "training") ------
    TRAINABLE = ('fp32', 'bf16x3')
    MIXED_PRECISIONS = {None: 0, 'bf16': 1}     # dsen2_model_set_train_precision

    def compile(self, optimizer='nadam', loss='mean_absolute_error', metrics=None, mixed_precision=None, *, loss_param=None,
                mask_nodata=False, ssim_weight=0.0, ssim_win=11, ssim_sigma=1.5, ssim_data_range=5.0):
        """keras Model.compile for the reference's recipe: optimizer 'nadam' or a training.Nadam, loss
        'mean_absolute_error' (MSE is always reported as the metric).  The optimizer state starts fresh.
        optimizer: 'nadam' (the default), 'adam', 'sgd', or a training.Nadam / Adam / SGD, each of which takes the keyword-only
        options clipnorm, clipvalue, weight_decay and decay_bias (training.Optimizer): clipping by the gradient's global norm over
        all weight tensors and by value, and decoupled weight decay on the convolution kernels.  A Nadam without options steps
        through the kernels it always did; every training path follows the optimiser, and last_grad_norm() reads the norm.
        loss: 'mean_absolute_error' / 'mae' (the default, the reference's), 'mean_squared_error' / 'mse', 'huber' or 'charbonnier'
        (losses.py has the table).  loss_param (keyword only): Huber's delta / Charbonnier's epsilon as a float32 > 0, required
        for those two — errors live in the reflectance / 2000 domain, where keras's delta = 1 would just be MSE / 2 — and refused
        for the others.  mask_nodata=True (keyword only): a pixel whose target is exactly 0 in every band carries no ground truth
        (the fill of a swath edge): it adds nothing to the loss, the metric or any gradient; the denominator stays the number of
        all elements.  Every training path follows these — train_on_batch (shards too), train_on_device_batch, fit,
        fit_corpus, data_parallel, emulate_world, augment — and so do evaluate, the validation passes and therefore
        logs['loss'] / ['val_loss'], ReduceLROnPlateau and ModelCheckpoint; 'mean_squared_error' stays the (masked) MSE.  Note
        that ReduceLROnPlateau's absolute min_delta=1e-6 is large beside an MSE in the normalised domain: lower it with loss='mse'.
        ssim_weight > 0 (keyword only) adds Zhao et al. 2017's term  ssim_weight * mean over all windows of (1 - SSIM)  to the loss,
        with its gradient on the GPU (include/dsen2_hip.h, "the SSIM loss term"): the window is metrics.ssim_window(ssim_win,
        ssim_sigma), ssim_win odd in 3..11, and c1 = (0.01 L)^2, c2 = (0.03 L)^2 with L = ssim_data_range in the normalised domain
        (5.0 = the metrics' 10000 / SCALE).  Under mask_nodata a window that holds a masked pixel adds nothing; the denominator
        stays the number of all windows.  The same paths follow it; logs['loss'] and ['val_loss'] are then the total the
        optimiser minimises, 'mean_squared_error' is unchanged.  Patches must be at least ssim_win on a side.  0 (the default):
        every bit as without the term.
        mixed_precision='bf16' (fp32 models only): the training step — fit, train_on_batch, gradients_device — runs its
        convolutions on bf16 operands with fp32 accumulation, the arithmetic of a precision='bf16' model; the weights, the
        optimizer state, the checkpoint, predict, evaluate and fit's validation pass stay fp32.  None: the model's own
        arithmetic."""
        from . import training, losses
        if self.precision not in self.TRAINABLE:
            raise ValueError('training needs an fp32 or a bf16x3 model (this one is %r)' % self.precision)
        if mixed_precision not in self.MIXED_PRECISIONS:
            raise ValueError("mixed_precision must be None or 'bf16', got %r" % (mixed_precision,))
        if mixed_precision is not None and self.precision != 'fp32':
            raise ValueError('mixed_precision=%r is an option of an fp32 model (this one is %r)' % (mixed_precision, self.precision))
        setting = losses.parse_ssim(losses.parse(loss, loss_param, mask_nodata), ssim_weight, ssim_win, ssim_sigma, ssim_data_range)
        if isinstance(optimizer, str):
            if optimizer.lower() not in training.OPTIMIZERS:
                raise ValueError("optimizer must be 'nadam', 'adam', 'sgd' or a dsen2_amd.training optimizer, got %r" % optimizer)
            optimizer = training.OPTIMIZERS[optimizer.lower()]()
        if not isinstance(optimizer, training.Optimizer):
            raise ValueError('optimizer must be a dsen2_amd.training.Nadam, Adam or SGD')
        if optimizer.weight_decay:
            training.decay_ranges(self.cin, self.cout, self.num_layers, self.feature_size, optimizer.decay_bias)    # (refused here, not at the first step)
        if self.precision == 'fp32':
            with torch.cuda.device(self.device):
                _lib.call('dsen2_model_set_train_precision', self._handle, self.MIXED_PRECISIONS[mixed_precision])
        with torch.cuda.device(self.device):
            _lib.call('dsen2_model_set_loss', self._handle, setting[0], setting[1], setting[2])
            ssim = losses.ssim_part(setting) or (0.0, 11, 1.5, 5.0)
            window, c1, c2 = losses.ssim_constants(ssim)
            _lib.call('dsen2_model_set_loss_ssim', self._handle, ssim[0], (ctypes.c_double * window.size)(*window.tolist()),
                      int(window.size), c1, c2)
        self.loss_setting = setting
        self.mixed_precision = mixed_precision
        self.optimizer = optimizer
        self.optimizer.reset()
        self._train = None
        self.stop_training = False

    def _train_state(self):
        if getattr(self, 'optimizer', None) is None:
            raise RuntimeError('compile() the model before training it')
        if self._train is None:
            count = self.count_params()
            kw = dict(dtype=torch.float32, device=self.device)
            flat = torch.empty(count, **kw)
            with torch.cuda.device(self.device):
                _lib.call('dsen2_model_get_weights', self._handle, _ptr(flat), _stream_ptr(self.device))
            # (SGD keeps its velocity in m and has no second moment)
            self._train = dict(flat=flat, grad=torch.empty(count, **kw), m=torch.zeros(count, **kw),
                               v=torch.zeros(count, **kw) if self.optimizer.KIND != 2 else None, loss2=torch.empty(2, **kw), ws=None,
                               # what a step through dsen2_optimizer_step keeps (built by the first such step: the options of an
                               # optimiser are as mutable as its lr, so the route is chosen step by step)
                               norm=None, norm_valid=False, opt_work=None, ranges=None)
        return self._train

    def _plain_nadam(self):
        """The optimiser is a Nadam without options: its step is dsen2_nadam_step / dsen2_nadam_step_shards, as it always was.
        Asked at every step: setting an option on the optimiser later moves the following steps to dsen2_optimizer_step."""
        from . import training
        return isinstance(self.optimizer, training.Nadam) and not self.optimizer.has_options()

    def _decay_range_array(self):
        """(n, ctypes array of 2 n unsigned) of the optimiser's decay ranges as its options stand NOW; (0, None) without weight
        decay.  Kept with the training state under the options it was made from."""
        from . import training
        opt = self.optimizer
        key = (bool(opt.weight_decay), bool(opt.decay_bias))
        st = self._train
        if st['ranges'] is None or st['ranges'][0] != key:
            if not opt.weight_decay:
                made = (0, None)
            else:
                ranges = training.decay_ranges(self.cin, self.cout, self.num_layers, self.feature_size, opt.decay_bias)
                made = (len(ranges), (ctypes.c_uint * (2 * len(ranges)))(*[int(x) for r in ranges for x in r]))
            st['ranges'] = (key, made)
        return st['ranges'][1]

    def _optimizer_desc(self, s):
        """The dsen2_optimizer_desc of the step whose scalars next_step() has returned as `s`."""
        opt = self.optimizer
        n, arr = self._decay_range_array()
        d = _lib.OptimizerDesc()
        d.kind = opt.KIND
        for k in ('lr', 'b1', 'b2', 'eps', 'mc_t', 'mc_t1', 'ms_new', 'ms_next', 'b2_pow_t', 'lr_t', 'momentum'):
            setattr(d, k, s.get(k, 0.0))
        d.nesterov = int(bool(s.get('nesterov', False)))
        d.clipnorm, d.clipvalue, d.weight_decay = opt.clipnorm, opt.clipvalue, opt.weight_decay
        d.n_ranges = n
        d.host_ranges = ctypes.cast(arr, ctypes.POINTER(ctypes.c_uint)) if n else None
        return d

    def last_grad_norm(self):
        """The global norm (over all weight tensors, before clipping) of the mean gradient of the last step, as the float64 the
        step's kernels left on the device: with or without clipnorm, so it can be looked at before a clipnorm is chosen.  Every
        step through dsen2_optimizer_step forms it — Adam, SGD, a Nadam with an option; a Nadam without options steps through
        the kernels it always did, which form none: RuntimeError then, and before the first step.  This read is the only call of
        the optimiser path that waits for the device."""
        st = self._train_state()
        if not st['norm_valid']:
            raise RuntimeError('no gradient norm: the last step was not one of Adam, SGD or a Nadam with clipnorm, clipvalue or '
                               'weight_decay (a Nadam without options forms none)')
        return float(st['norm'].cpu().numpy()[0])

    def _optimizer_step(self, g, stride, counts, g_mean=None):
        """THE optimiser step: on the gradient vector g (counts None), or on the count-weighted mean of the rows g[r] of `stride`
        floats with counts[r] samples each.  A Nadam without options takes the entries it always took (dsen2_nadam_step,
        dsen2_nadam_step_shards: the same launches, the same bits); everything else is dsen2_optimizer_step.  A refused call is
        not a step.  Then the device repack."""
        st = self._train_state()
        opt = self.optimizer
        count = st['flat'].numel()
        before = opt.step_state()
        s = opt.next_step()
        try:
            with torch.cuda.device(self.device):
                if self._plain_nadam():
                    scalars = (s['lr'], s['b1'], s['b2'], s['eps'], s['mc_t'], s['mc_t1'], s['ms_new'], s['ms_next'], s['b2_pow_t'])
                    if counts is None:
                        _lib.call('dsen2_nadam_step', _ptr(st['flat']), _ptr(g), _ptr(st['m']), _ptr(st['v']), count, *scalars,
                                  _stream_ptr(self.device))
                    else:
                        _lib.call('dsen2_nadam_step_shards', _ptr(st['flat']), _ptr(g), stride, len(counts),
                                  (ctypes.c_int * len(counts))(*counts), _ptr(g_mean), _ptr(st['m']), _ptr(st['v']), count, *scalars,
                                  _stream_ptr(self.device))
                    st['norm_valid'] = False
                else:
                    if counts is None:
                        stride, counts = count, [1]
                    desc = self._optimizer_desc(s)
                    if st['norm'] is None:
                        st['norm'] = torch.zeros(1, dtype=torch.float64, device=self.device)
                    # the norm is always asked for (one more read of the gradient): last_grad_norm() works without clipnorm
                    need = ctypes.c_size_t(0)
                    _lib.call('dsen2_optimizer_step_work_bytes', ctypes.byref(desc), count, len(counts), int(g_mean is not None), 1,
                              ctypes.byref(need))
                    if st['opt_work'] is None or st['opt_work'].numel() < need.value:
                        st['opt_work'] = None
                        st['opt_work'] = torch.empty(need.value, dtype=torch.uint8, device=self.device)
                    work = st['opt_work']
                    st['norm_valid'] = False
                    _lib.call('dsen2_optimizer_step', ctypes.byref(desc), _ptr(st['flat']), _ptr(g), stride, len(counts),
                              (ctypes.c_int * len(counts))(*counts), _ptr(g_mean), _ptr(st['m']), _ptr(st['v']), count, _ptr(work),
                              work.numel(), _ptr(st['norm']), _stream_ptr(self.device))
                    st['norm_valid'] = True
        except Exception:
            opt.set_step_state(before)          # a refused call is not a step
            raise
        self.set_weights_device(st['flat'])

    def train_workspace_bytes(self, n, h, w):
        out = ctypes.c_size_t(0)
        _lib.call('dsen2_model_train_workspace_bytes', self._handle, n, h, w, ctypes.byref(out))
        return out.value

    def gradients_device(self, xs, y, grad, loss2, out=None, workspace=None):
        """dsen2_model_gradients on device tensors: xs as forward_device, y [n,cout,h,w]; grad [num_params] and loss2 [2]
        receive the keras-flat gradient and (mae, mse); out (optional) the forward output."""
        if self.precision not in self.TRAINABLE:
            raise ValueError('training needs an fp32 or a bf16x3 model (this one is %r)' % self.precision)
        n, _, h, w = xs[0].shape
        for x, c in zip(xs, self.bands):
            if tuple(x.shape) != (n, c, h, w) or x.dtype != torch.float32 or not x.is_contiguous() or x.device != self.device:
                raise ValueError('input must be a contiguous float32 %s tensor of shape %r' % (self.device, (n, c, h, w)))
        if len(xs) != len(self.bands):
            raise ValueError('expected %d inputs, got %d' % (len(self.bands), len(xs)))
        if tuple(y.shape) != (n, self.cout, h, w) or y.dtype != torch.float32 or not y.is_contiguous() or y.device != self.device:
            raise ValueError('target must be a contiguous float32 %s tensor of shape %r, got %r'
                             % (self.device, (n, self.cout, h, w), tuple(y.shape)))
        if grad.numel() != self.count_params() or not grad.is_contiguous() or loss2.numel() < 2:
            raise ValueError('grad must hold num_params floats, loss2 two')
        if out is not None:
            out = self._check_out(out, n, h, w)
        if workspace is None:
            need = self.train_workspace_bytes(n, h, w)
            st = self._train if self._train is not None else {}
            if st.get('ws') is None or st['ws'].numel() < need:
                st['ws'] = None
                st['ws'] = torch.empty(need, dtype=torch.uint8, device=self.device)
            workspace = st['ws']
        with torch.cuda.device(self.device):
            _lib.call('dsen2_model_gradients', self._handle, _ptr(xs[0]), _ptr(xs[1]),
                      _ptr(xs[2]) if len(xs) == 3 else ctypes.c_void_p(0), _ptr(y), _ptr(out), _ptr(grad), _ptr(loss2),
                      n, h, w, _ptr(workspace), workspace.numel(), _stream_ptr(self.device))
        return out

    def set_weights_device(self, flat):
        """New keras-flat weights from a float32 device tensor, repacked on the device.  A model being trained continues from
        them: get_weights_flat() returns them and the next optimizer step updates them (as after set_weights_flat)."""
        if flat.numel() != self.count_params() or flat.dtype != torch.float32 or not flat.is_contiguous() or \
                flat.device != self.device:
            raise ValueError('flat must be a contiguous float32 %s tensor of %d values' % (self.device, self.count_params()))
        with torch.cuda.device(self.device):
            _lib.call('dsen2_model_set_weights_device', self._handle, _ptr(flat), _stream_ptr(self.device))
            if self._train is not None and flat.data_ptr() != self._train['flat'].data_ptr():
                self._train['flat'].copy_(flat)      # a model being trained continues from the new weights (as set_weights_flat)

    def nadam_update(self, grad):
        """One optimizer step on the training weights with gradient `grad` (device tensor), then the device repack."""
        self._optimizer_step(grad, None, None)

    def _to_device(self, arrays, shapes):
        out = []
        for a, shp in zip(arrays, shapes):
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != shp:
                raise ValueError('array of shape %r where %r is expected' % (a.shape, shp))
            out.append(torch.from_numpy(a).to(self.device))
        return out

    # -- sharded steps: gradient accumulation on one GPU, data-parallel training on several ---------------------------------
    def _shard_rows(self, k):
        """[k, count + 2 (+ up to 3 floats of padding)] float32 device rows of a sharded step, kept with the training state: the
        gradient, then loss2.  The padding makes the row length a multiple of 4 floats, here and after an all-gather, so that
        dsen2_nadam_step_shards takes 16-byte accesses; it is never read."""
        st = self._train_state()
        count = st['flat'].numel()
        rows = st.get('rows')
        if rows is None or rows.shape[0] != k:
            stride = -(-(count + 2) // 4) * 4
            rows = st['rows'] = torch.empty((k, stride), dtype=torch.float32, device=self.device)
        return rows

    def nadam_update_shards(self, buf, counts, g_mean=None):
        """One optimizer step on the count-weighted mean of the gradient vectors buf[r, :num_params] (float32 device rows, counts[r]
        samples behind row r; a row whose count is 0 is never read), added in row order: dsen2_nadam_step_shards, then the device
        repack.  The step of train_on_batch(shards=...) and of every rank of a data-parallel group alike.  g_mean (optional,
        [num_params]) receives the averaged gradient."""
        st = self._train_state()
        count = st['flat'].numel()
        counts = [int(c) for c in counts]
        if buf.dim() != 2 or buf.shape[0] != len(counts) or buf.shape[1] < count or buf.dtype != torch.float32 or \
                buf.device != self.device or buf.stride(1) != 1 or (len(counts) > 1 and buf.stride(0) < count):
            raise ValueError('buf must hold %d float32 %s rows of at least %d values, got %r strides %r'
                             % (len(counts), self.device, count, tuple(buf.shape), buf.stride()))
        if g_mean is not None and (g_mean.numel() != count or g_mean.dtype != torch.float32 or not g_mean.is_contiguous() or
                                   g_mean.device != self.device):
            raise ValueError('g_mean must be a contiguous float32 %s tensor of %d values' % (self.device, count))
        self._optimizer_step(buf, max(buf.stride(0), count), counts, g_mean)

    @staticmethod
    def weighted_loss(loss2, counts):
        """[sum n_r mae_r / n, sum n_r mse_r / n] in float64, added in shard order; a shard without samples is not read."""
        total = float(sum(counts))
        acc = [0.0, 0.0]
        for l2, c in zip(loss2, counts):
            if c > 0:
                acc[0] += float(c) * float(l2[0])
                acc[1] += float(c) * float(l2[1])
        return [acc[0] / total, acc[1] / total]

    @staticmethod
    def _check_augment_ops(augment_ops, n, h, w):
        """One op 0..7 per sample of the batch as an int32 array (None stays None: no augmentation)."""
        if augment_ops is None:
            return None
        ops = np.ascontiguousarray(augment_ops, dtype=np.int32)
        if ops.shape != (n,) or (n and (ops.min() < 0 or ops.max() > 7)):
            raise ValueError('augment_ops must hold one op 0..7 for each of the %d samples, got %r' % (n, np.asarray(augment_ops).tolist()))
        if h != w:
            raise ValueError('augmentation turns every sample by its own op: it needs square patches, got %dx%d' % (h, w))
        return ops

    def _augment_device(self, tensors, ops):
        """Every tensor [n, c, h, w] turned sample by sample: D_ops[s] of sample s (ops None: as they are)."""
        if ops is None:
            return tensors
        ops_dev = torch.from_numpy(ops).to(self.device)
        return [dihedral(t, ops=ops_dev) for t in tensors]

    def _step_on_shards(self, fetch, counts, mine=None, augment_ops=None):
        """One step on a global batch cut into contiguous shards of counts[r] samples.  fetch(first, n) returns (x, y) of samples
        [first, first + n) of the batch: host arrays, which are uploaded here, or float32 device tensors, which are used as they
        are (fit_corpus: cut on the device, the ops already applied).  mine = None: every shard is computed here, one after the other (gradient
        accumulation; the one-process restatement of a data-parallel step).  mine = r: this process is rank r of a group of
        len(counts) and computes shard r alone; the rows are all-gathered.  Either way the same rows reach the same kernel in the
        same order.  augment_ops (or None): the checked ops of the GLOBAL batch, sliced like the samples.  Returns the
        count-weighted [loss, mean_squared_error] of the batch."""
        from . import dist
        count = self._train_state()['flat'].numel()
        rows = self._shard_rows(len(counts) if mine is None else 1)
        first = 0
        for r, n in enumerate(counts):
            if n > 0 and mine in (None, r):
                x, y = fetch(first, n)
                _, _, h, w = np.shape(x[0])
                if isinstance(y, torch.Tensor):
                    xs, yd = list(x), y
                else:
                    xs = self._to_device(x, [(n, c, h, w) for c in self.bands])
                    yd = self._to_device([y], [(n, self.cout, h, w)])[0]
                if augment_ops is not None:
                    *xs, yd = self._augment_device(xs + [yd], self._check_augment_ops(augment_ops[first:first + n], n, h, w))
                row = rows[r if mine is None else 0]
                self.gradients_device(xs, yd, row[:count], row[count:count + 2])
            first += n
        if mine is not None:
            rows = dist.all_gather_rows(rows[0])
        self.nadam_update_shards(rows, counts)
        return self.weighted_loss(rows[:, count:count + 2].cpu().numpy().astype(np.float64), counts)

    def _shard_counts(self, n, shards):
        from . import dist
        if isinstance(shards, (int, np.integer)):
            if shards < 1:
                raise ValueError('shards must be at least 1, got %d' % shards)
            return [dist.shard_range(n, r, int(shards))[1] for r in range(int(shards))]
        counts = [int(c) for c in shards]
        if not counts or min(counts) < 0 or sum(counts) != n:
            raise ValueError('the shard counts %r must be non-negative and add up to the batch of %d' % (counts, n))
        return counts

    def train_on_batch(self, x, y, shards=None, augment_ops=None):
        """keras Model.train_on_batch: one Nadam step on the batch; returns [loss, mean_squared_error] of the batch
        before the step.
        augment_ops (default None: the data as given): one op 0..7 per sample (include/dsen2_hip.h, "dihedral": a flip and / or a
        rotation by a multiple of 90 degrees); the inputs and the target of sample s are turned by D_ops[s] on the device after the
        upload — the step is bit for bit the step on data turned on the host.  Square patches only.  With shards, every shard
        takes its slice of the ops.
        shards (default None: the whole batch in one pass): an integer k, or a list of counts that add up to the batch — the
        batch is cut into contiguous shards (k: dist.shard_range's cut, the one a k-rank data-parallel run makes), each goes
        through gradients_device on its own, and ONE step follows on the count-weighted mean of the shard gradients, added in
        shard order in double (dsen2_nadam_step_shards).  Gradient accumulation: a global batch larger than the workspace allows;
        and the exact one-process restatement of a data-parallel step.  shards=1 is the plain step, bit for bit; k > 1 differs
        from it by the summation order only.  The losses returned are the count-weighted float64 means of the shards'."""
        st = self._train_state()
        if len(x) != len(self.bands):
            raise ValueError('expected %d inputs, got %d' % (len(self.bands), len(x)))
        n, _, h, w = np.shape(x[0])
        ops = self._check_augment_ops(augment_ops, n, h, w)
        if shards is not None:
            counts = self._shard_counts(n, shards)
            x = [np.ascontiguousarray(a, dtype=np.float32) for a in x]
            y = np.ascontiguousarray(y, dtype=np.float32)
            if y.shape != (n, self.cout, h, w) or any(a.shape != (n, c, h, w) for a, c in zip(x, self.bands)):
                raise ValueError('inputs %r and target %r do not describe one batch' % ([a.shape for a in x], y.shape))
            return self._step_on_shards(lambda first, m: ([a[first:first + m] for a in x], y[first:first + m]), counts,
                                        augment_ops=ops)
        xs = self._to_device(x, [(n, c, h, w) for c in self.bands])
        yd = self._to_device([y], [(n, self.cout, h, w)])[0]
        *xs, yd = self._augment_device(xs + [yd], ops)
        self.gradients_device(xs, yd, st['grad'], st['loss2'])
        self.nadam_update(st['grad'])
        loss = st['loss2'].cpu().numpy().astype(np.float64)
        return [float(loss[0]), float(loss[1])]

    def train_on_device_batch(self, xs, y, loss_out=None):
        """train_on_batch for a batch that is already on the device (float32 NCHW tensors, as gradients_device takes them):
        gradients_device, then nadam_update.  [loss, mean_squared_error] of the batch before the step stay on the device: in
        loss_out (a float32 device tensor of two values) when given, else in the training state's own pair, which the next step
        overwrites; the tensor is returned.  Nothing is copied to the host and nothing synchronises."""
        st = self._train_state()
        loss2 = st['loss2'] if loss_out is None else loss_out
        if loss2.dtype != torch.float32 or loss2.numel() != 2 or not loss2.is_contiguous() or loss2.device != self.device:
            raise ValueError('loss_out must be a contiguous float32 %s tensor of two values' % (self.device,))
        self.gradients_device(list(xs), y, st['grad'], loss2)
        self.nadam_update(st['grad'])
        return loss2

    def evaluate(self, x, y, batch_size=None, verbose=0):
        """keras Model.evaluate: [loss, mean_squared_error] over all samples (predict(), then float64 means)."""
        y = np.asarray(y, dtype=np.float32)
        pred = self.predict(x, batch_size=batch_size, verbose=verbose)
        if pred.shape != y.shape:
            raise ValueError('target of shape %r where %r is expected' % (y.shape, pred.shape))
        from . import losses
        return losses.host_loss(pred, y, self._loss_setting())

    def _loss_setting(self):
        """The setting of the last compile() (losses.py: (kind, param, mask_mode), with the SSIM part behind it when its weight is
        > 0); the MAE, unmasked, for a model that was never compiled."""
        from . import losses
        return getattr(self, 'loss_setting', losses.DEFAULT)

    def _means_of_triples(self, triples, mine):
        """[sum rho / elements, sum d^2 / elements] of the ranks' float64 (sum rho, sum d^2, elements) rows, added in rank order.
        mine = r: this process holds row r alone and the rows are all-gathered first; None: it holds them all."""
        if mine is not None:
            from . import dist
            triples = dist.all_gather_rows(torch.from_numpy(triples[mine]).to(self.device)).cpu().numpy()
        sa = sq = cnt = 0.0
        for t in triples:
            sa, sq, cnt = sa + t[0], sq + t[1], cnt + t[2]
        return [float(sa / cnt), float(sq / cnt)]

    def _evaluate_shards(self, x, y, batch_size, world, mine=None):
        """[loss, mean_squared_error] over all samples as a data-parallel group of `world` ranks forms it: shard r =
        dist.shard_range(n, r, world) of the samples is predicted on its own and gives float64 (sum |e|, sum e^2, elements) on the
        host, as evaluate() forms them; the triples are added in rank order.  mine = None: every shard here, one after the other;
        mine = r: shard r alone, the triples all-gathered.  The same number on every rank."""
        from . import dist, losses
        y = np.asarray(y, dtype=np.float32)
        n = y.shape[0]
        triples = np.zeros((world, 3), np.float64)
        for r in range(world):
            if mine in (None, r):
                first, cnt = dist.shard_range(n, r, world)
                pred = self.predict([a[first:first + cnt] for a in x], batch_size=batch_size)
                triples[r] = losses.host_sums(pred, y[first:first + cnt], self._loss_setting())
        return self._means_of_triples(triples, mine)

    def _data_parallel_plan(self, data_parallel, emulate_world):
        """None: the plain fit.  Else (world, mine): the sharded steps of a group of `world` ranks, as rank `mine` of the process
        group, or (mine None, emulate_world) with every shard computed in this process.  Without either keyword the process
        group is not looked at."""
        if not data_parallel and emulate_world is None:
            return None
        from . import dist
        rank, world = dist.rank_world()
        if emulate_world is not None:
            if not data_parallel or world > 1 or int(emulate_world) < 1:
                raise ValueError('emulate_world restates a data-parallel run in ONE process: it needs data_parallel=True, a world '
                                 'of at least 1 and no process group of more than one rank')
            return (int(emulate_world), None) if int(emulate_world) > 1 else None
        return (world, rank) if data_parallel and world > 1 else None

    def _data_parallel_start(self, seed):
        """Every rank continues from rank 0's weights and draws rank 0's permutations: the keras-flat vector and the shuffle seed
        (drawn here on rank 0 when None) travel in one broadcast.  Returns the seed."""
        from . import dist
        rank, _ = dist.rank_world()
        payload = None
        if rank == 0:
            if seed is None:
                seed = int(np.random.SeedSequence().generate_state(1, np.uint64)[0] >> np.uint64(1))
            payload = np.concatenate([self.get_weights_flat(), np.array([seed], np.uint64).view(np.float32)])
        payload = dist.broadcast_weights(payload, self.count_params() + 2, device=self.device)
        self.set_weights_flat(payload[:-2])
        return int(payload[-2:].view(np.uint64)[0])

    def _sums_device(self, pred, target, out, setting=None):
        """The body of the two methods below.  setting None: dsen2_abs_sq_error_sums over the flat pair, which never forms a
        count; else dsen2_loss_sums for (kind, param, mask) over an NCHW pair, its three numbers parked behind its scratch."""
        for t in (pred, target):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device or tuple(t.shape) != tuple(pred.shape) \
                    or (setting is not None and t.dim() != 4):
                raise ValueError('pred and target must be contiguous float32 %s %stensors of one shape'
                                 % (self.device, 'NCHW ' if setting is not None else ''))
        if out.dtype != torch.float64 or out.numel() != 2 or not out.is_contiguous() or out.device != self.device:
            raise ValueError('out must be a contiguous float64 %s tensor of two values' % (self.device,))
        need = ctypes.c_size_t(0)
        _lib.call('dsen2_abs_sq_error_sums_workspace_bytes' if setting is None else 'dsen2_loss_sums_workspace_bytes', ctypes.byref(need))
        size = need.value + (0 if setting is None else 24)
        work = self._error_work
        if work is None or work.numel() < size:
            work = self._error_work = torch.empty(size, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            if setting is None:
                _lib.call('dsen2_abs_sq_error_sums', _ptr(pred), _ptr(target), pred.numel(), _ptr(work), work.numel(), _ptr(out),
                          _stream_ptr(self.device))
                return out
            out3 = work[need.value:need.value + 24].view(torch.float64)
            n, c, h, w = pred.shape
            kind, param, mask = setting
            _lib.call('dsen2_loss_sums', _ptr(pred), _ptr(target), n, c, h * w, kind, param, mask, _ptr(work), need.value, _ptr(out3),
                      _stream_ptr(self.device))
        out.copy_(out3[:2])
        return out

    def abs_sq_error_sums_device(self, pred, target, out):
        """out[0 .. 1] = (sum |pred - target|, sum (pred - target)^2) in float64, formed on the device in an order that the number
        of elements alone fixes (dsen2_abs_sq_error_sums).  pred, target: contiguous float32 device tensors of one shape; out: a
        contiguous float64 device tensor of two values.  Nothing is copied to the host and nothing synchronises."""
        return self._sums_device(pred, target, out)

    def loss_sums_device(self, pred, target, out):
        """abs_sq_error_sums_device for the compiled loss: out[0 .. 1] = (sum rho, sum d^2) over the unmasked elements of an NCHW
        [n, c, h, w] pair (dsen2_loss_sums; its third number, the unmasked count, stays in the scratch).  With the default
        setting this IS abs_sq_error_sums_device."""
        from . import losses
        setting = self._loss_setting()
        kind, param, mask = losses.pointwise(setting)
        self._sums_device(pred, target, out, None if (kind, mask) == (0, 0) else (kind, param, mask))
        if losses.ssim_part(setting):
            # out[0] = sum rho + ssim_fold * sum (1 - q), as losses.host_sums forms it: a float64 product, then a float64 sum
            s3 = self._ssim_sums_device(pred, target, setting)
            out[0:1].add_(s3[0:1] * losses.ssim_fold(setting, tuple(pred.shape)))
        return out

    def _ssim_sums_device(self, pred, target, setting):
        """{ sum (1 - q), Nw, unmasked windows } of the compiled SSIM term over an NCHW pair (dsen2_ssim_loss_sums), a float64
        device tensor of three values behind the call's scratch; the next call overwrites it."""
        from . import losses
        window, c1, c2 = losses.ssim_constants(losses.ssim_part(setting))
        need = ctypes.c_size_t(0)
        _lib.call('dsen2_ssim_loss_sums_workspace_bytes', ctypes.byref(need))
        work = getattr(self, '_ssim_work', None)
        if work is None or work.numel() < need.value + 24 or work.device != self.device:
            work = self._ssim_work = torch.empty(need.value + 24, dtype=torch.uint8, device=self.device)
        out3 = work[need.value:need.value + 24].view(torch.float64)
        n, c, h, w = pred.shape
        with torch.cuda.device(self.device):
            _lib.call('dsen2_ssim_loss_sums', _ptr(pred), _ptr(target), n, c, h, w, (ctypes.c_double * window.size)(*window.tolist()),
                      int(window.size), c1, c2, setting[2], _ptr(work), need.value, _ptr(out3), _stream_ptr(self.device))
        return out3

    def _validation_rows(self, corpus, table, rows):
        """The device validation pass over the sample rows `table` of `corpus`: chunks of preferred_batch crops are cut
        (corpus.batch: op 0, _check_validation_crops refuses any other; divisor SCALE), go through forward_device — what predict runs — and chunk j's pair of error
        sums lands in rows[j].  Everything is enqueued; nothing is read."""
        from . import training
        chunk = self._validation_chunk(corpus)
        for j, i0 in enumerate(range(0, table.shape[0], chunk)):
            xs, y = corpus.batch(table[i0:i0 + chunk], divisor=training.SCALE)
            self.loss_sums_device(self.forward_device(xs), y, rows[j])

    def _validation_chunk(self, corpus):
        return max(1, int(self.preferred_batch(corpus.patch, corpus.patch)))

    @staticmethod
    def _check_validation_crops(corpus, validation_crops):
        table = corpus.check_table(validation_crops)
        if table.shape[0] == 0:
            raise ValueError('validation_crops holds no sample')
        if (table[:, 3] != 0).any():
            raise ValueError('validation is never augmented: every row of validation_crops must have op 0 (corpus.validation_table '
                             'draws such rows), got ops %r' % (sorted(set(table[:, 3].tolist())),))
        return table

    def _validate_crops(self, corpus, table, plan):
        """[val_loss, val_mean_squared_error] of the crops `table` under a data-parallel plan (world, mine), as _evaluate_shards
        forms them: shard r = dist.shard_range(n, r, world) of the rows gives the float64 triple (sum |e|, sum e^2, elements) —
        its chunks' pairs added in chunk order on the host — and the triples are added in rank order.  mine None: every shard
        here; mine = r: shard r alone, the triples all-gathered."""
        from . import dist
        world, mine = plan
        elements = self.cout * corpus.patch * corpus.patch
        chunk = self._validation_chunk(corpus)
        triples = np.zeros((world, 3), np.float64)
        for r in range(world):
            if mine in (None, r):
                first, cnt = dist.shard_range(table.shape[0], r, world)
                if cnt > 0:
                    rows = torch.empty((-(-cnt // chunk), 2), dtype=torch.float64, device=self.device)
                    self._validation_rows(corpus, table[first:first + cnt], rows)
                    sa = sq = 0.0
                    for row in rows.cpu().numpy():
                        sa, sq = sa + row[0], sq + row[1]
                    triples[r] = (sa, sq, float(cnt * elements))
        return self._means_of_triples(triples, mine)

    def _end_epoch(self, epoch, epochs, sums, count, validation_data, batch_size, plan, callbacks, history, verbose, val=None):
        """The end of an epoch of fit and of fit_corpus alike: the epoch's losses from `sums` (the float64 sums of samples x batch
        loss) over `count` samples, the validation pass (sharded like the steps under a data-parallel plan; val: its two numbers
        where fit_corpus has formed them on the device), the log line, the callbacks, the History entry, and under a process
        group the check that every rank holds the same weights."""
        logs = {'loss': sums[0] / count, 'mean_squared_error': sums[1] / count}
        if val is not None:
            logs['val_loss'], logs['val_mean_squared_error'] = val
        elif validation_data is not None:
            if plan is None:
                vl = self.evaluate(validation_data[0], validation_data[1], batch_size=batch_size)
            else:
                vl = self._evaluate_shards(validation_data[0], validation_data[1], batch_size, plan[0], plan[1])
            logs['val_loss'], logs['val_mean_squared_error'] = vl
        logs['lr'] = self.optimizer.lr
        if verbose:
            sys.stdout.write('\rEpoch %d/%d ' % (epoch + 1, epochs) +
                             ' '.join('%s %.4e' % kv for kv in logs.items()) + '\n')
        for cb in callbacks:
            cb.on_epoch_end(epoch, logs)
        history.append(epoch, logs)
        if plan is not None and plan[1] is not None:
            from . import dist
            dist.assert_replicas_identical(self._train['flat'])

    def fit(self, x=None, y=None, batch_size=32, epochs=1, verbose=1, callbacks=None, validation_data=None, shuffle=True,
            initial_epoch=0, seed=None, data_parallel=False, emulate_world=None, augment=False):
        """keras Model.fit: a fresh permutation each epoch when `shuffle`, the last partial batch kept, the epoch loss the
        sample-weighted mean of the batch losses.  Returns a training.History (loss, mean_squared_error, val_loss,
        val_mean_squared_error, lr).
        data_parallel=True under a torch.distributed process group of N > 1 ranks (dist.init_from_env): `batch_size` is the GLOBAL
        batch; every rank holds all of x and y, starts from rank 0's weights and shuffle seed, computes the gradient of its
        dist.shard_range share of each batch, all-gathers the gradient vectors and takes the same step on their count-weighted mean,
        added in rank order (nadam_update_shards): the weights stay bit-identical on every rank, which is checked after every
        epoch.  The validation set is sharded the same way and its float64 sums are added in rank order, so logs, callbacks and
        stop_training act alike on every rank.  Without a group (or with one rank) it is the plain fit, as is data_parallel=False
        always.  emulate_world=W (with data_parallel=True, one process): the same steps and validation sums with the W shards
        computed here one after the other — what a W-rank run computes, bit for bit.
        augment=True (default off; square patches): every training sample of every step is flipped and / or rotated by a
        multiple of 90 degrees, inputs and target alike, on the device (train_on_batch(augment_ops=...)).  The ops of a step are
        training.AugmentOps(seed).draw(batch): a generator derived from `seed` but separate from the shuffle's, so the
        permutations are those of the un-augmented fit.  Under data_parallel every rank draws the ops of the GLOBAL batch from
        the broadcast seed and takes its shard's slice.  Validation is never augmented."""
        from . import training
        if getattr(y, 'class_masked', False) or (validation_data is not None and getattr(validation_data[1], 'class_masked', False)):
            training.check_masked_target(self._loss_setting(), True, 'fit')
        plan = self._data_parallel_plan(data_parallel, emulate_world)
        x = [np.ascontiguousarray(a, dtype=np.float32) for a in x]
        y = np.ascontiguousarray(y, dtype=np.float32)
        count = y.shape[0]
        if any(a.shape[0] != count for a in x):
            raise ValueError('inputs and target hold different numbers of samples')
        self._train_state()
        callbacks = list(callbacks or [])
        history = training.History()
        for cb in callbacks:
            cb.set_model(self)
            cb.on_train_begin()
        if plan is not None:
            seed = self._data_parallel_start(seed)
        rng = np.random.default_rng(seed)
        aug = training.AugmentOps(seed) if augment else None
        self.stop_training = False
        for epoch in range(initial_epoch, epochs):
            order = rng.permutation(count) if shuffle else np.arange(count)
            sums = np.zeros(2)
            for i0 in range(0, count, batch_size):
                idx = order[i0:i0 + batch_size]
                ops = aug.draw(len(idx)) if aug is not None else None
                if plan is None:
                    r = self.train_on_batch([a[idx] for a in x], y[idx], augment_ops=ops)
                else:
                    r = self._step_on_shards(lambda first, m: ([a[idx[first:first + m]] for a in x], y[idx[first:first + m]]),
                                             self._shard_counts(len(idx), plan[0]), plan[1], augment_ops=ops)
                sums += np.asarray(r) * len(idx)
                if verbose:
                    sys.stdout.write('\rEpoch %d/%d %d/%d loss %.4e' % (epoch + 1, epochs, min(i0 + batch_size, count), count,
                                                                     sums[0] / min(i0 + batch_size, count)))
                    sys.stdout.flush()
            self._end_epoch(epoch, epochs, sums, count, validation_data, batch_size, plan, callbacks, history, verbose)
            if self.stop_training:
                break
        return history

    def fit_corpus(self, corpus, batch_size, steps_per_epoch, epochs=1, validation_data=None, seed=None, augment=False,
                   callbacks=None, initial_epoch=0, verbose=1, shards=None, data_parallel=False, emulate_world=None,
                   validation_crops=None, masks=None):
        """fit from a corpus.TileCorpus: an epoch is steps_per_epoch batches of batch_size fresh crops, drawn by ONE
        corpus.CorpusSampler(corpus, seed, augment) and cut on the device (corpus.batch: one launch per step, the dihedral ops of
        `augment` included).  Per step the host draws the table, uploads it through page-locked memory and enqueues
        train_on_device_batch; the step's two losses go into a device [steps_per_epoch, 2] buffer that is read ONCE per epoch —
        no other copy and no synchronisation happen inside an epoch.  The epoch loss is fit's formula: the float64 sum of
        batch_size * loss over the steps, in step order, divided by the number of samples (all batches are equal: the mean).
        Validation (validation_data: host arrays, e.g. corpus.validation_arrays), logs, callbacks, the History returned and
        stop_training are exactly fit's.
        Sharded steps: shards=K cuts every batch as train_on_batch(shards=K) does (gradient accumulation);
        data_parallel / emulate_world are fit's: every rank draws the table of the GLOBAL batch from the broadcast seed and cuts
        its dist.shard_range slice from its own copy of the corpus; the rest is _step_on_shards, which reads each step's losses
        (these modes synchronise once per step, as fit does).
        masks (default None): CorpusSampler's — one packed origin bitmap per tile (corpus.origin_masks()[0]); training crops are
        drawn from valid origins only (free of blank cells, outside the hold-out), tiles still uniform.
        validation_crops (default None; not together with validation_data: ValueError): an int32 [k, 4] sample table, e.g.
        corpus.validation_table(...).  Validation then stays on the device: after the last step of an epoch the table is cut in
        chunks of preferred_batch crops (corpus.batch, divisor SCALE), every chunk goes through forward_device on the model's own
        plan — what predict runs: fp32 for an fp32 model, also under mixed_precision — and dsen2_abs_sq_error_sums writes chunk
        j's (sum |e|, sum e^2) into row j of a device float64 [chunks, 2] buffer, which is read in the SAME synchronising read as
        the epoch's training losses; nothing else reaches the host.  The host adds the rows in chunk order and divides by the
        element count.  Under data_parallel / emulate_world the table is sharded by dist.shard_range as _evaluate_shards shards
        its samples, and the ranks' (sum |e|, sum e^2, elements) triples are all-gathered and added in rank order."""
        from . import training
        from .corpus import CorpusSampler
        if getattr(corpus, 'class_masked', False):
            training.check_masked_target(self._loss_setting(), True, 'fit_corpus')
        plan = self._data_parallel_plan(data_parallel, emulate_world)
        if plan is not None and shards is not None:
            raise ValueError('shards is the one-process cut of a batch: it cannot be combined with data_parallel')
        batch_size, steps = int(batch_size), int(steps_per_epoch)
        if batch_size < 1 or steps < 1:
            raise ValueError('batch_size and steps_per_epoch must be at least 1, got %d and %d' % (batch_size, steps))
        if corpus.device != self.device or tuple(c for c in self.bands) != tuple(s[1] for s in corpus.output_shapes(1)[0]) or \
                self.cout != corpus.cout:
            raise ValueError('the corpus (%s, run_60=%r) does not feed this model (%s, bands %r)'
                             % (corpus.device, corpus.run_60, self.device, tuple(self.bands)))
        if validation_crops is not None and validation_data is not None:
            raise ValueError('validation_data (host arrays) and validation_crops (a sample table, validated on the device) exclude '
                             'each other')
        val_table = None if validation_crops is None else self._check_validation_crops(corpus, validation_crops)
        self._train_state()
        callbacks = list(callbacks or [])
        history = training.History()
        for cb in callbacks:
            cb.set_model(self)
            cb.on_train_begin()
        if plan is not None:
            seed = self._data_parallel_start(seed)
        sampler = CorpusSampler(corpus, seed, augment, masks=masks)
        sharded = plan is not None or shards is not None
        chunks = 0
        if val_table is not None and plan is None:
            chunks = -(-val_table.shape[0] // self._validation_chunk(corpus))
            val_elements = float(val_table.shape[0] * self.cout * corpus.patch * corpus.patch)
        # one device buffer for everything an epoch reports: the steps' float32 loss pairs, then the validation chunks' float64
        # pairs (8 bytes per loss pair: the float64 rows start on a multiple of 8)
        report = torch.empty((0 if sharded else steps) * 8 + chunks * 16, dtype=torch.uint8, device=self.device)
        if chunks:
            val_rows = report[report.numel() - chunks * 16:].view(torch.float64).view(chunks, 2)
        if not sharded:
            losses = report[:steps * 8].view(torch.float32).view(steps, 2)
            tables = torch.empty((steps, batch_size, 4), dtype=torch.int32).pin_memory()      # one slot per step of an epoch: a
            tables_dev = torch.empty((steps, batch_size, 4), dtype=torch.int32, device=self.device)   # slot is free again after the
        count = steps * batch_size                                                           # epoch's read of the losses
        self.stop_training = False
        for epoch in range(initial_epoch, epochs):
            sums = np.zeros(2)
            for i in range(steps):
                table = sampler.draw(batch_size)
                if not sharded:
                    tables[i].numpy()[...] = table
                    tables_dev[i].copy_(tables[i], non_blocking=True)
                    xs, y = corpus.batch(table, table_dev=tables_dev[i])
                    self.train_on_device_batch(xs, y, loss_out=losses[i])
                else:
                    counts = self._shard_counts(batch_size, shards if plan is None else plan[0])
                    r = self._step_on_shards(lambda first, m: corpus.batch(table[first:first + m]), counts,
                                             None if plan is None else plan[1])
                    sums += np.asarray(r) * batch_size
                if verbose:
                    sys.stdout.write('\rEpoch %d/%d %d/%d' % (epoch + 1, epochs, (i + 1) * batch_size, count))
                    sys.stdout.flush()
            val = None
            if chunks:
                self._validation_rows(corpus, val_table, val_rows)                # enqueued behind the last step
            if not sharded or chunks:
                host = report.cpu().numpy()                                       # the epoch's one read
                if not sharded:
                    for r in host[:steps * 8].view(np.float32).reshape(steps, 2).astype(np.float64):
                        sums += r * batch_size
                if chunks:
                    sa = sq = 0.0
                    for row in host[host.size - chunks * 16:].view(np.float64).reshape(chunks, 2):
                        sa, sq = sa + row[0], sq + row[1]
                    val = [float(sa / val_elements), float(sq / val_elements)]
            elif val_table is not None:
                val = self._validate_crops(corpus, val_table, plan)
            self._end_epoch(epoch, epochs, sums, count, validation_data, batch_size, plan, callbacks, history, verbose, val=val)
            if self.stop_training:
                break
        return history

    def get_weights_flat(self):
        """The current weights in keras-flat order (host float32)."""
        if self._train is not None:
            flat = self._train['flat']
        else:
            flat = torch.empty(self.count_params(), dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.call('dsen2_model_get_weights', self._handle, _ptr(flat), _stream_ptr(self.device))
        return flat.cpu().numpy()

    def save_weights(self, path):
        """A flat .npy in keras-flat order (weights.load_flat reads it; DSen2_20 picks it up in place of a missing .hdf5)."""
        np.save(path, self.get_weights_flat())

    def __del__(self):
        try:
            if self._handle:
                _lib.load().dsen2_model_destroy(self._handle)
                self._handle = ctypes.c_void_p(0)
        except Exception:
            pass


def s2model(input_shape, num_layers=32, feature_size=256, device=None, precision='fp32'):
    """utils/DSen2Net.py:18 — same positional arguments and defaults.  precision='bf16' / 'bf16x3' run the residual-block
    convolutions on the bf16 matrix cores (fp32 accumulate, exact fp32 residual stream; PRECISIONS above)."""
    return S2Model(input_shape, num_layers, feature_size, device=device, precision=precision)


def to_blocked(x_nhwc):
    """[n,h,w,c] -> the blocked layout of the bf16 kernels [n, c/8, h, w, 8] (a torch reshuffle, test helper)."""
    n, h, w, c = x_nhwc.shape
    return x_nhwc.reshape(n, h, w, c // 8, 8).permute(0, 3, 1, 2, 4).contiguous()


def from_blocked(x_blk):
    n, b, h, w, e = x_blk.shape
    return x_blk.permute(0, 2, 3, 1, 4).reshape(n, h, w, b * e).contiguous()


def split_f32(x):
    """fp32 NHWC CUDA tensor -> (hi, lo): blocked int16 tensors [n, c/8, h, w, 8] (include/dsen2_hip.h: dsen2_split_f32)."""
    x = x.contiguous()
    n, h, w, c = x.shape
    hi = torch.empty((n, c // 8, h, w, 8), dtype=torch.int16, device=x.device)
    lo = torch.empty_like(hi)
    with torch.cuda.device(x.device):
        _lib.call('dsen2_split_f32', _ptr(x), _ptr(hi), _ptr(lo), n, h, w, c, _stream_ptr(x.device))
    return hi, lo


def join_f32(hi, lo):
    n, b, h, w, e = hi.shape
    out = torch.empty((n, h, w, b * e), dtype=torch.float32, device=hi.device)
    with torch.cuda.device(hi.device):
        _lib.call('dsen2_join_f32', _ptr(hi), _ptr(lo), _ptr(out), n, h, w, b * e, _stream_ptr(hi.device))
    return out


def split3_f32(x):
    """fp32 NHWC CUDA tensor -> (hx, lo16): hx int16 [n, 2, c/8, h, w, 8] (plane 0 = hi, plane 1 = xl = bf16(x - hi)) and the
    low halves int16 [n, c/8, h, w, 8] (include/dsen2_hip.h: dsen2_split3_f32) — the residual stream of a 'bf16x3' model."""
    x = x.contiguous()
    n, h, w, c = x.shape
    hx = torch.empty((n, 2, c // 8, h, w, 8), dtype=torch.int16, device=x.device)
    lo = torch.empty((n, c // 8, h, w, 8), dtype=torch.int16, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call('dsen2_split3_f32', _ptr(x), _ptr(hx), _ptr(lo), n, h, w, c, _stream_ptr(x.device))
    return hx, lo


def join3_f32(hx, lo):
    """The exact inverse of split3_f32: (hx, lo16) -> fp32 NHWC (include/dsen2_hip.h: dsen2_join3_f32)."""
    n, _, b, h, w, e = hx.shape
    out = torch.empty((n, h, w, b * e), dtype=torch.float32, device=hx.device)
    with torch.cuda.device(hx.device):
        _lib.call('dsen2_join3_f32', _ptr(hx), _ptr(lo), _ptr(out), n, h, w, b * e, _stream_ptr(hx.device))
    return out


def conv3x3_wgrad_bf16x3(a_planes, g_planes, scale=1.0):
    """Kernel-level entry point of the bf16x3 weight gradient (include/dsen2_hip.h: dsen2_conv3x3_wgrad_bf16x3): a_planes,
    g_planes int16 [n, 2, feat/8, h, w, 8] two-plane operand tensors.  Returns (dw [3, 3, feat, feat] HWIO, db [feat])."""
    n, _, b, h, w, e = a_planes.shape
    feat = b * e
    if tuple(g_planes.shape) != tuple(a_planes.shape) or not a_planes.is_contiguous() or not g_planes.is_contiguous():
        raise ValueError('a_planes and g_planes must be contiguous tensors of the same shape')
    dw = torch.empty((3, 3, feat, feat), dtype=torch.float32, device=a_planes.device)
    db = torch.empty(feat, dtype=torch.float32, device=a_planes.device)
    with torch.cuda.device(a_planes.device):
        _lib.call('dsen2_conv3x3_wgrad_bf16x3', _ptr(a_planes), _ptr(g_planes), _ptr(dw), _ptr(db), n, h, w, feat, float(scale),
                  _stream_ptr(a_planes.device))
    return dw, db


def bf16_plane_f32(x):
    """fp32 NHWC CUDA tensor -> the one-plane blocked bf16 operand tensor int16 [n, c/8, h, w, 8] of conv3x3_wgrad_bf16: the hi
    plane of split_f32, (u + 0x8000) >> 16 of every bit pattern (exact for values that already are bf16)."""
    return split_f32(x)[0]


def conv3x3_wgrad_bf16(a_plane, g_plane, scale=1.0):
    """Kernel-level entry point of the bf16 weight gradient of the mixed-precision training step (include/dsen2_hip.h:
    dsen2_conv3x3_wgrad_bf16): a_plane, g_plane int16 / bfloat16 [n, feat/8, h, w, 8] one-plane blocked operand tensors.  Returns
    (dw [3, 3, feat, feat] HWIO, db [feat])."""
    n, b, h, w, e = a_plane.shape
    feat = b * e
    if tuple(g_plane.shape) != tuple(a_plane.shape) or not a_plane.is_contiguous() or not g_plane.is_contiguous() or \
            a_plane.element_size() != 2 or g_plane.element_size() != 2:
        raise ValueError('a_plane and g_plane must be contiguous 16-bit tensors of the same shape')
    dw = torch.empty((3, 3, feat, feat), dtype=torch.float32, device=a_plane.device)
    db = torch.empty(feat, dtype=torch.float32, device=a_plane.device)
    with torch.cuda.device(a_plane.device):
        _lib.call('dsen2_conv3x3_wgrad_bf16', _ptr(a_plane), _ptr(g_plane), _ptr(dw), _ptr(db), n, h, w, feat, float(scale),
                  _stream_ptr(a_plane.device))
    return dw, db


WGRAD_KINDS = {'fp32': 0, 'bf16x3': 1, 'bf16': 2}


def conv3x3_wgrad_geometry(kind, n, h, w, ca, cg=None):
    """What a launch of a weight-gradient kernel does at a shape (include/dsen2_hip.h: dsen2_conv3x3_wgrad_geometry; host code,
    needs no device).  kind 'fp32' (ca, cg as dsen2_conv3x3_wgrad takes them), 'bf16x3' or 'bf16' (ca = cg = feat).  Returns
    (tiles, splits, workspace_floats): run s of the splits covers tiles [tiles * s // splits, tiles * (s + 1) // splits)."""
    cg = ca if cg is None else cg
    tiles, splits, floats = ctypes.c_longlong(0), ctypes.c_int(0), ctypes.c_size_t(0)
    _lib.call('dsen2_conv3x3_wgrad_geometry', WGRAD_KINDS[kind], n, h, w, ca, cg, ctypes.byref(tiles), ctypes.byref(splits),
              ctypes.byref(floats))
    return tiles.value, splits.value, floats.value


def conv3x3_first_planes(xs, kernel_hwio, bias, precision):
    """Kernel-level entry point of the first convolution of a 'bf16' (precision 1) / 'bf16x3' (2) model on the bf16 matrix
    cores (include/dsen2_hip.h: dsen2_conv3x3_first_planes).  xs: the two or three NCHW float32 CUDA inputs (4 + 6 (+ 2)
    bands); kernel_hwio (3, 3, 10 | 12, feat).  Returns the residual stream as the model holds it: precision 1 (hi, lo) int16
    [n, feat/8, h, w, 8]; precision 2 (hx, lo16) with hx int16 [n, 2, feat/8, h, w, 8] (plane 0 = hi, plane 1 = xl)."""
    kernel_hwio = np.ascontiguousarray(kernel_hwio, np.float32)
    bias = np.ascontiguousarray(bias, np.float32)
    feat = kernel_hwio.shape[3]
    n, _, h, w = xs[0].shape
    dev = xs[0].device
    xs = [x.contiguous() for x in xs]
    if precision == 2:
        out = torch.empty((n, 2, feat // 8, h, w, 8), dtype=torch.int16, device=dev)
    else:
        out = torch.empty((n, feat // 8, h, w, 8), dtype=torch.int16, device=dev)
    out2 = torch.empty((n, feat // 8, h, w, 8), dtype=torch.int16, device=dev)
    with torch.cuda.device(dev):
        _lib.call('dsen2_conv3x3_first_planes', _ptr(xs[0]), _ptr(xs[1]), _ptr(xs[2]) if len(xs) == 3 else ctypes.c_void_p(0),
                  xs[0].shape[1], xs[1].shape[1], xs[2].shape[1] if len(xs) == 3 else 0,
                  kernel_hwio.ctypes.data_as(_lib.c_float_p), bias.ctypes.data_as(_lib.c_float_p), int(feat), int(precision),
                  _ptr(out), _ptr(out2), n, h, w, _stream_ptr(dev))
    return out, out2


def conv3x3_body_bf16x3(x_planes, kernel_hwio, bias, epilogue=0, res_hx=None, res_lo=None, res_scale=RES_SCALE):
    """Kernel-level entry point of the bf16x3 body convolution.  x_planes: int16 (bf16 bit patterns) [n, 2, feat/8, h, w, 8].
    epilogue 0: returns relu(conv + bias) as such a two-plane tensor.  epilogue 1: updates the stream (res_hx, res_lo; see
    split3_f32) in place and returns it.  epilogue 3: returns the updated stream as fp32 NHWC."""
    n, _, blocks, h, w, _ = x_planes.shape
    feat = blocks * 8
    kernel_hwio = np.ascontiguousarray(kernel_hwio, np.float32)
    bias = np.ascontiguousarray(bias, np.float32)
    out = None
    if epilogue == 0:
        out = torch.empty((n, 2, feat // 8, h, w, 8), dtype=torch.int16, device=x_planes.device)
    elif epilogue == 3:
        out = torch.empty((n, h, w, feat), dtype=torch.float32, device=x_planes.device)
    with torch.cuda.device(x_planes.device):
        _lib.call('dsen2_conv3x3_body_bf16x3', _ptr(x_planes.contiguous()), kernel_hwio.ctypes.data_as(_lib.c_float_p),
                  bias.ctypes.data_as(_lib.c_float_p), _ptr(res_hx), _ptr(res_lo), _ptr(out), n, h, w, feat, int(epilogue),
                  float(res_scale), _stream_ptr(x_planes.device))
    return (res_hx, res_lo) if epilogue == 1 else out


def conv3x3_body_bf16(x_bf16, kernel_hwio, bias, epilogue=0, res_hi=None, res_lo=None, res_scale=RES_SCALE):
    """Kernel-level entry point of the bf16 body convolution: x_bf16 NHWC torch.bfloat16 CUDA tensor (reshuffled to
    the kernel's blocked layout here).  epilogue 0: returns relu(conv + bias) as bf16 NHWC.  epilogue 1: updates the
    residual stream's blocked planes (res_hi, res_lo; see split_f32) in place and returns them.  epilogue 3:
    returns the updated residual stream as fp32 NHWC (planes untouched)."""
    n, h, w, feat = x_bf16.shape
    kernel_hwio = np.ascontiguousarray(kernel_hwio, np.float32)
    bias = np.ascontiguousarray(bias, np.float32)
    xb = to_blocked(x_bf16)
    out = None
    if epilogue == 0:
        out = torch.empty((n, feat // 8, h, w, 8), dtype=torch.bfloat16, device=x_bf16.device)
    elif epilogue == 3:
        out = torch.empty((n, h, w, feat), dtype=torch.float32, device=x_bf16.device)
    with torch.cuda.device(x_bf16.device):
        _lib.call('dsen2_conv3x3_body_bf16', _ptr(xb), kernel_hwio.ctypes.data_as(_lib.c_float_p),
                  bias.ctypes.data_as(_lib.c_float_p), _ptr(res_hi), _ptr(res_lo), _ptr(out), n, h, w, feat, int(epilogue),
                  float(res_scale), _stream_ptr(x_bf16.device))
    if epilogue == 1:
        return res_hi, res_lo
    return from_blocked(out) if epilogue == 0 else out


def conv3x3_nhwc(x, kernel_hwio, bias, epilogue=0, aux=None, res_scale=RES_SCALE, ref=False):
    """Single-layer entry point (kernel-level parity tests): x NHWC float32 CUDA tensor.  ref=True runs the
    one-tile-per-workgroup kernel (dsen2_conv3x3_nhwc_ref), the independent structure for cross-checks."""
    n, h, w, cin = x.shape
    kernel_hwio = np.ascontiguousarray(kernel_hwio, np.float32)
    bias = np.ascontiguousarray(bias, np.float32)
    cout = kernel_hwio.shape[3]
    if epilogue == 2:
        out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device)
    else:
        out = torch.empty((n, h, w, cout), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call('dsen2_conv3x3_nhwc_ref' if ref else 'dsen2_conv3x3_nhwc', _ptr(x), kernel_hwio.ctypes.data_as(_lib.c_float_p),
                  bias.ctypes.data_as(_lib.c_float_p), _ptr(aux), _ptr(out), n, h, w, cin, cout, int(epilogue),
                  float(res_scale), _stream_ptr(x.device))
    return out
