#!/usr/bin/env python3
"""Digests of the training step, for refactors of it that must not change a bit: one JSON line per mode and case.

    python tools/train_step_digest.py > after.jsonl        (and the same at the commit before; the two files must be equal)

Modes: fp32, bf16x3, fp32 with compile(mixed_precision='bf16').  Cases: the nets of tests/test_gpu_memory_contract.py's
test_gradients (the smallest shapes at which each path of the step can still go wrong) and the multi-tile split-K batch of
tests/test_gpu_train_amp.py.  Per line: train_workspace_bytes; sha256 of out, grad and loss2 of one gradients_device; of the
flat weights after one train_on_batch and of forward_device after it; the same two after set_weights_flat of fresh weights on
the trained model and another step (the master vector follows a load); fp32 only: of the gradient after
compile(mixed_precision='bf16') and compile(mixed_precision=None) (the training state dropped and rebuilt twice).
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsen2_amd import training, weights  # noqa: E402
from dsen2_amd.DSen2Net import s2model  # noqa: E402

MODES = {'fp32': ('fp32', None), 'bf16x3': ('bf16x3', None), 'fp32-amp': ('fp32', 'bf16')}
CASES = [((4, 6), 2, 128, 3, 21, 37), ((4, 6, 2), 1, 256, 1, 9, 21), ((4, 6), 1, 128, 2, 1, 1), ((4, 6), 0, 128, 2, 5, 7),
         ((4, 6), 1, 128, 20, 21, 37)]


def sha(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run(mode, bands, d, feat, n, h, w):
    precision, mixed = MODES[mode]
    dev = torch.device('cuda', 0)
    m = s2model(tuple((c, None, None) for c in bands), num_layers=d, feature_size=feat, device=dev, precision=precision)
    m.set_weights_flat(weights.random_he_uniform(sum(bands), bands[-1], d, feat, seed=1, bias_scale=0.05))
    m.compile(training.Nadam(lr=1e-3), mixed_precision=mixed)
    rng = np.random.default_rng(7)
    xs = [rng.uniform(0, 0.5, (n, c, h, w)).astype(np.float32) for c in bands]
    y = rng.uniform(0, 0.5, (n, bands[-1], h, w)).astype(np.float32)
    xs_d, y_d = [torch.from_numpy(a).to(dev) for a in xs], torch.from_numpy(y).to(dev)
    grad, loss2 = torch.empty(m.count_params(), device=dev), torch.empty(2, device=dev)

    def step():
        m.train_on_batch(xs, y)
        return dict(weights=sha(m.get_weights_flat()), forward=sha(m.forward_device(xs_d)))

    res = dict(mode=mode, case=[list(bands), d, feat, n, h, w], train_workspace_bytes=m.train_workspace_bytes(n, h, w))
    out = m.gradients_device(xs_d, y_d, grad, loss2, out=torch.empty(n, bands[-1], h, w, device=dev))
    res.update(out=sha(out), grad=sha(grad), loss2=sha(loss2), step=step())
    m.set_weights_flat(weights.random_he_uniform(sum(bands), bands[-1], d, feat, seed=2, bias_scale=0.05))
    res['step_after_load'] = step()
    if mode == 'fp32':
        m.compile(training.Nadam(lr=1e-3), mixed_precision='bf16')
        m.compile(training.Nadam(lr=1e-3), mixed_precision=None)
        m.gradients_device(xs_d, y_d, grad, loss2)
        res['grad_after_recompile'] = sha(grad)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    for mode in MODES:
        for case in CASES:
            run(mode, *case)
