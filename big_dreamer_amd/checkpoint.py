"""Host helpers of checkpoint and resume ("Checkpoint and resume"): capture and restore of the process's random
generators in a form ``torch.load(..., weights_only=True)`` accepts, the file names of a run's checkpoints, an atomic file
write and the pruning of older checkpoints.  No kernels and no device work except reading / setting the device generator's
state; everything else runs without a GPU."""
from __future__ import annotations

import os
import random
import re
from typing import Any, Callable, Dict, List, Optional

import numpy as np
import torch


# ------------------------------------------------------------------------------------------------ generators
def capture_generators(device: Optional[torch.device] = None) -> Dict[str, Any]:
    """The states of the four generators a run draws from outside the engine's Philox streams, as tensors and plain
    ints / floats (nothing that a ``weights_only`` load would refuse):
      torch_cpu    -- torch.get_rng_state(): module initialisation, torch.rand on the host;
      torch_device -- torch.cuda.get_rng_state(device): the composed acting path, PlaNet's exploration noise (absent when
                      `device` is None or not a CUDA device);
      numpy        -- np.random.get_state(): the replay's index draws (memory._sample_idx);
      python       -- random.getstate()."""
    out: Dict[str, Any] = {"torch_cpu": torch.get_rng_state().clone()}
    if device is not None and torch.device(device).type == "cuda":
        out["torch_device"] = torch.cuda.get_rng_state(torch.device(device)).clone()
    name, keys, pos, has_gauss, cached = np.random.get_state()
    out["numpy"] = {"name": str(name), "keys": torch.from_numpy(np.asarray(keys, dtype=np.int64).copy()), "pos": int(pos),
                    "has_gauss": int(has_gauss), "cached_gaussian": float(cached)}
    version, words, gauss_next = random.getstate()
    out["python"] = {"version": int(version), "words": torch.tensor(words, dtype=torch.int64),
                     "gauss_next": None if gauss_next is None else float(gauss_next)}
    return out


def restore_generators(state: Dict[str, Any], device: Optional[torch.device] = None) -> None:
    """Set the generators to what ``capture_generators`` returned.  ``torch_device`` is restored on `device` when both are
    there."""
    torch.set_rng_state(state["torch_cpu"].to(dtype=torch.uint8, device="cpu"))
    if "torch_device" in state and device is not None and torch.device(device).type == "cuda":
        torch.cuda.set_rng_state(state["torch_device"].to(dtype=torch.uint8, device="cpu"), torch.device(device))
    n = state["numpy"]
    np.random.set_state((n["name"], n["keys"].numpy().astype(np.uint32), int(n["pos"]), int(n["has_gauss"]),
                         float(n["cached_gaussian"])))
    p = state["python"]
    random.setstate((int(p["version"]), tuple(int(w) for w in p["words"].tolist()), p["gauss_next"]))


def check_extra(extra: Optional[Dict[str, Any]]) -> Dict[str, Any]:
    """The caller's part of a checkpoint: a flat dict of ints, floats and strings."""
    extra = dict(extra or {})
    for k, v in extra.items():
        if not isinstance(k, str) or isinstance(v, bool) or not isinstance(v, (int, float, str)):
            raise ValueError(f"checkpoint extra: {k!r}: {v!r} -- keys are strings, values ints, floats or strings")
    return extra


def read_run_state(path: str) -> Dict[str, Any]:
    """The ``run_state`` of a checkpoint ``Dreamer.save`` wrote, read with a loader that executes nothing from the file.
    ValueError for a checkpoint without one (the reference's files, and files older than this key)."""
    d = torch.load(path, map_location="cpu", weights_only=True)
    rs = d.get("run_state") if isinstance(d, dict) else None
    if rs is None:
        raise ValueError(f"{path} holds no run_state (the reference's checkpoints and those written before run_state "
                         "existed carry weights and optimisers only): it can be loaded with models=, not resumed")
    return rs


# ------------------------------------------------------------------------------------------------ files
_KINDS = {"models": ".pth", "experience": ".npz"}
_NAME = re.compile(r"^(models|experience)_(\d+)(?:_rank(\d+))?\.(pth|npz)$")


def _path(directory: str, kind: str, step: int, rank: int, world_size: int) -> str:
    suffix = f"_rank{int(rank)}" if int(world_size) > 1 else ""
    return os.path.join(directory, f"{kind}_{int(step)}{suffix}{_KINDS[kind]}")


def models_path(directory: str, step: int, rank: int = 0, world_size: int = 1) -> str:
    """``<dir>/models_<step>.pth``; ``models_<step>_rank<r>.pth`` when world_size > 1 (every rank writes its own: the
    generator states differ per rank)."""
    return _path(directory, "models", step, rank, world_size)


def experience_path(directory: str, step: int, rank: int = 0, world_size: int = 1) -> str:
    """``<dir>/experience_<step>.npz``; ``experience_<step>_rank<r>.npz`` when world_size > 1 (every rank collects its
    own experience)."""
    return _path(directory, "experience", step, rank, world_size)


def for_rank(path: str, rank: int, world_size: int) -> str:
    """The file of `rank` next to `path`: with world_size > 1, ``..._rank<q>.ext`` becomes ``..._rank<rank>.ext`` (a user
    names one rank's file, every rank loads its own); a name without a rank suffix, and any name when world_size is 1, is
    returned as it is."""
    if int(world_size) <= 1:
        return path
    head, name = os.path.split(path)
    return os.path.join(head, re.sub(r"_rank\d+(\.[^.]+)$", rf"_rank{int(rank)}\1", name))


def atomic_write(path: str, write: Callable[[Any], None]) -> None:
    """Call ``write(fh)`` on a temporary file in the directory of `path`, flush it to the disk, then ``os.replace`` it onto
    `path`: a reader, or a machine reset in the middle of a save, finds under `path` the earlier file or the whole new
    one, never a truncated one.  If `write` raises, the temporary file is removed and `path` is untouched."""
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        with open(tmp, "wb") as fh:
            write(fh)
            fh.flush()
            os.fsync(fh.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.remove(tmp)
        except OSError:
            pass
        raise


def list_checkpoints(directory: str) -> Dict[int, List[str]]:
    """{step: [file names]} of this project's ``models_*`` / ``experience_*`` files in `directory` (all ranks)."""
    found: Dict[int, List[str]] = {}
    for name in sorted(os.listdir(directory)):
        m = _NAME.match(name)
        if m and _KINDS[m.group(1)] == "." + m.group(4) and os.path.isfile(os.path.join(directory, name)):
            found.setdefault(int(m.group(2)), []).append(name)
    return found


def prune(directory: str, keep: int, rank: Optional[int] = None) -> List[str]:
    """Remove the ``models_<step>[_rank<r>].pth`` / ``experience_<step>[_rank<r>].npz`` files of all but the newest `keep`
    steps; returns the removed paths.  ``keep <= 0`` removes nothing, and no file with any other name is touched.
    `rank`: look at that rank's ``_rank<r>`` files only (data-parallel runs: every rank prunes its own, so no rank removes
    a file another is still writing); None: every file of a step.  A temporary file a killed save left behind
    (``<name>.tmp<pid>``) is not a checkpoint and stays."""
    if keep <= 0 or not os.path.isdir(directory):
        return []
    found = list_checkpoints(directory)
    if rank is not None:
        found = {step: mine for step, names in found.items()
                 if (mine := [n for n in names if _NAME.match(n).group(3) == str(int(rank))])}
    removed = []
    for step in sorted(found)[:-keep]:
        for name in found[step]:
            path = os.path.join(directory, name)
            os.remove(path)
            removed.append(path)
    return removed

