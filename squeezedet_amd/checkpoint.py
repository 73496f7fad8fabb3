"""Checkpoints of a training run (the reference's tf.train.Saver over tf.global_variables(), src/train.py:240,328-330).

A checkpoint of step S is a PAIR of files:
  * ``<train_dir>/model.ckpt-<S>.npz``: every model variable, frozen ones included, through weights.save_params -- the file
    eval.py polls for and demo.py --weights reads;
  * ``<train_dir>/state/step-<S>.npz``: what continuing needs on top -- the trainer's and the reader's state_dict() and a few
    run settings (``extra``).  It sits in a sub-directory on purpose: eval.latest_checkpoint globs '*-*.npz' in the directory
    itself and must never pick a state file up.
A run that keeps an EMA of its weights (train.py --ema_decay) adds ``<train_dir>/ema/model.ckpt-<S>.npz``: the model file with the
trainable variables taken from the average -- written before the raw model file, pruned with its pair, read by eval.py --ema.
Both are written under a hidden temporary name and moved into place with os.replace, because eval.py polls while training
writes; the model file goes last, so a checkpoint that eval.py can see is always complete.
"""
import glob
import json
import os

import numpy as np

from . import weights

MODEL_FMT, STATE_FMT = "model.ckpt-%d.npz", os.path.join("state", "step-%d.npz")
EMA_DIR = "ema"


def _steps(paths):
    out = set()
    for p in paths:
        s = os.path.basename(p)[:-len(".npz")].split("-")[-1]
        if s.isdigit():
            out.add(int(s))
    return out


def steps(train_dir):
    """Sorted steps that have BOTH files."""
    a = _steps(glob.glob(os.path.join(train_dir, "model.ckpt-*.npz")))
    b = _steps(glob.glob(os.path.join(train_dir, "state", "step-*.npz")))
    return sorted(a & b)


def latest(train_dir):
    """The largest step that has both its files, or None."""
    s = steps(train_dir)
    return s[-1] if s else None


def paths(train_dir, step):
    return os.path.join(train_dir, MODEL_FMT % step), os.path.join(train_dir, STATE_FMT % step)


def _flatten(prefix, d):
    return {prefix + k: np.asarray(v) for k, v in d.items()}


def save(train_dir, step, model, trainer, reader, extra=None, keep=0):
    """Writes the pair of step `step`; keep > 0 prunes all but the newest `keep` pairs.  Returns the model file's path."""
    step = int(step)
    model_path, state_path = paths(train_dir, step)
    os.makedirs(os.path.dirname(state_path), exist_ok=True)
    tr_state = trainer.state_dict()             # (flushes the trainer: a pending divergence is raised BEFORE anything is written)
    names = tr_state.pop("names")
    tr_state["names_json"] = json.dumps(names)
    tr_state["shapes_json"] = json.dumps(tr_state.pop("shapes"))
    arrays = dict(_flatten("trainer/", tr_state))
    arrays.update(_flatten("reader/", reader.state_dict()))
    arrays["extra_json"] = np.asarray(json.dumps(dict(extra or {}, step=step)))
    tmp = os.path.join(os.path.dirname(state_path), ".tmp-%d.npz" % os.getpid())
    np.savez(tmp, **arrays)
    os.replace(tmp, state_path)
    if getattr(trainer, "flat_ema", None) is not None:      # (--ema_decay: ahead of the raw model file, so a visible checkpoint has it)
        path = ema_path(train_dir, step)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        tmp = os.path.join(os.path.dirname(path), ".tmp-%d.npz" % os.getpid())
        weights.save_params(tmp, dict(model.params, **trainer.ema_params()))
        os.replace(tmp, path)
    tmp = os.path.join(train_dir, ".tmp-%d.npz" % os.getpid())
    weights.save_params(tmp, model)
    os.replace(tmp, model_path)
    if keep and keep > 0:
        for s in steps(train_dir)[:-int(keep)]:
            for p in paths(train_dir, s):
                os.remove(p)
            if os.path.exists(ema_path(train_dir, s)):
                os.remove(ema_path(train_dir, s))
    return model_path


def ema_path(train_dir, step):
    """The EMA weights of step `step` (a run with --ema_decay): every model variable, the trainable ones averaged.  In a
    sub-directory, like the state file: eval.latest_checkpoint's '*-*.npz' glob over <train_dir> must not pick it up."""
    return os.path.join(train_dir, EMA_DIR, MODEL_FMT % int(step))


def ema_of(model_path):
    """<dir>/model.ckpt-<S>.npz -> <dir>/ema/model.ckpt-<S>.npz (eval.py --ema on a file)."""
    return os.path.join(os.path.dirname(model_path), EMA_DIR, os.path.basename(model_path))


def load(train_dir, step, model, trainer, reader):
    """Restores the pair of step `step` into a model, its trainer and a reader built as the saving run built them.  Returns
    the ``extra`` dict (with ``step``)."""
    model_path, state_path = paths(train_dir, int(step))
    model.load_params(weights.load_params(model_path))            # all variables, the frozen ones too
    with np.load(state_path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    tr = {k[len("trainer/"):]: (v.item() if v.ndim == 0 else v) for k, v in d.items() if k.startswith("trainer/")}
    tr["names"], tr["shapes"] = json.loads(str(tr.pop("names_json"))), json.loads(str(tr.pop("shapes_json")))
    trainer.load_state_dict(tr)
    reader.load_state_dict({k[len("reader/"):]: (v.item() if v.ndim == 0 else v) for k, v in d.items() if k.startswith("reader/")})
    return json.loads(str(d["extra_json"]))


def read_extra(train_dir, step):
    with np.load(paths(train_dir, int(step))[1], allow_pickle=False) as z:
        return json.loads(str(z["extra_json"]))
