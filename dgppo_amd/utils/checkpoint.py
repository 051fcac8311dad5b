"""Weights-only reader / writer for the `{actor,Vl,Vh}.pkl` files (dgppo/algo/informarl_lagr.py:311-327,
informarl.py:459-470): a flax-named tree of arrays.

The reference loads them with plain `pickle.load`; `test.py --path` is user-supplied, so this build never does that.
`load_tree` runs a `pickle.Unpickler` whose `find_class` resolves ONLY the globals a tree of arrays needs and raises
`pickle.UnpicklingError` for anything else — nothing named in the file is imported or called:

  * numpy's array reconstruction (`_reconstruct`, `ndarray`, `dtype`, `scalar`, `_frombuffer`),
  * `collections.OrderedDict`,
  * flax's `FrozenDict` (read as a plain dict), and
  * `jax._src.array._reconstruct_array` (how a `jax.Array` pickles itself: numpy's own reduce tuple plus two state
    dicts) — rebuilt as the numpy array it wraps, so a checkpoint written by the reference loads without jax.
"""
from __future__ import annotations

import collections
import io
import os
import pickle
from typing import Any, BinaryIO, List, Optional

import numpy as np

try:                                    # numpy >= 2 moved the C helpers
    import numpy._core as _np_core
    import numpy._core.multiarray  # noqa: F401
    import numpy._core.numeric  # noqa: F401
except ImportError:                     # pragma: no cover
    import numpy.core as _np_core
_np_multiarray = _np_core.multiarray


def _frozen_dict(*args, **kwargs) -> dict:
    """flax.core.frozen_dict.FrozenDict(mapping) -> dict"""
    return dict(*args, **kwargs)


def _jax_reconstruct_array(fun, args, arr_state, aval_state):
    """jax._src.array._reconstruct_array(fun, args, arr_state, aval_state): `fun(*args)` is numpy's reduce of the host
    copy; the rest (weak_type, named_shape) has no meaning for a weight."""
    if fun is not _np_multiarray._reconstruct:
        raise pickle.UnpicklingError("jax array payload is not a numpy reconstruction")
    arr = fun(*args)
    arr.__setstate__(arr_state)
    return arr


def _numpy_globals() -> dict:
    """numpy pickles name its helpers under numpy.core.* (numpy 1.x) or numpy._core.* (numpy 2.x): accept both spellings."""
    out = {("numpy", "ndarray"): np.ndarray, ("numpy", "dtype"): np.dtype}
    helpers = {"multiarray": ("_reconstruct", "scalar"), "numeric": ("_frombuffer",)}
    for sub, names in helpers.items():
        mod = getattr(_np_core, sub)
        for name in names:
            fn = getattr(mod, name, None)
            if fn is not None:
                out[(f"numpy.core.{sub}", name)] = fn
                out[(f"numpy._core.{sub}", name)] = fn
    return out


_ALLOWED = {
    **_numpy_globals(),
    ("collections", "OrderedDict"): collections.OrderedDict,
    ("flax.core.frozen_dict", "FrozenDict"): _frozen_dict,
    ("jax._src.array", "_reconstruct_array"): _jax_reconstruct_array,
}


class _TreeUnpickler(pickle.Unpickler):
    def find_class(self, module: str, name: str) -> Any:
        fn = _ALLOWED.get((module, name))
        if fn is None:
            raise pickle.UnpicklingError(f"refusing to resolve global '{module}.{name}': checkpoints may only contain "
                                         f"dicts of numpy (or jax) arrays")
        return fn

    def persistent_load(self, pid):     # no external object references in a weights file
        raise pickle.UnpicklingError("persistent ids are not allowed in a checkpoint")


def _check_tree(tree, path="") -> None:
    if isinstance(tree, dict):
        for k, v in tree.items():
            if not isinstance(k, str):
                raise pickle.UnpicklingError(f"checkpoint key {path}/{k!r} is not a string")
            _check_tree(v, f"{path}/{k}")
    elif isinstance(tree, np.ndarray):
        if tree.dtype.hasobject:
            raise pickle.UnpicklingError(f"checkpoint leaf {path} has an object dtype")
    elif not isinstance(tree, (np.generic, int, float)):
        raise pickle.UnpicklingError(f"checkpoint leaf {path} is a {type(tree).__name__}, expected an array")


def load_tree(f: BinaryIO):
    """-> nested dict of numpy arrays.  Raises pickle.UnpicklingError on anything that is not one."""
    tree = _TreeUnpickler(f).load()
    _check_tree(tree)
    return tree


def loads_tree(data: bytes):
    return load_tree(io.BytesIO(data))


def save_tree(tree, f: BinaryIO) -> None:
    """the reference's on-disk format: pickle of the nested dict with numpy leaves."""
    _check_tree(tree)
    pickle.dump(tree, f)


# ---- the full training state: one tree per file, written atomically ({log_dir}/resume/{step}.pkl) ----
# It goes through the same writer and reader as the weights: dicts with string keys, numpy arrays, ints and floats.
# Generators are stored as the numbers that define them, strings as uint8 arrays.

def encode_str(s: str) -> np.ndarray:
    return np.frombuffer(s.encode("utf-8"), dtype=np.uint8).copy()


def decode_str(a) -> str:
    return np.asarray(a, dtype=np.uint8).tobytes().decode("utf-8", "replace")


def generator_state(gen: np.random.Generator) -> dict:
    """a PCG64 `np.random.Generator` -> its two 128-bit integers and the buffered half draw, as plain ints"""
    st = gen.bit_generator.state
    if st["bit_generator"] != "PCG64":
        raise TypeError(f"only PCG64 generators are checkpointed, not {st['bit_generator']}")
    return {"state": int(st["state"]["state"]), "inc": int(st["state"]["inc"]), "has_uint32": int(st["has_uint32"]),
            "uinteger": int(st["uinteger"])}


def set_generator_state(gen: np.random.Generator, d: dict) -> None:
    gen.bit_generator.state = {"bit_generator": "PCG64", "state": {"state": int(d["state"]), "inc": int(d["inc"])},
                               "has_uint32": int(d["has_uint32"]), "uinteger": int(d["uinteger"])}


def global_numpy_state() -> dict:
    """the process-global `np.random` (MT19937): key uint32[624], position and the cached gaussian"""
    name, key, pos, has_gauss, cached = np.random.get_state()
    assert name == "MT19937", name
    return {"key": np.asarray(key, dtype=np.uint32).copy(), "pos": int(pos), "has_gauss": int(has_gauss),
            "cached_gaussian": float(cached)}


def set_global_numpy_state(d: dict) -> None:
    key = np.asarray(d["key"], dtype=np.uint32)
    if key.shape != (624,):
        raise ValueError(f"MT19937 key has shape {key.shape}, expected (624,)")
    np.random.set_state(("MT19937", key, int(d["pos"]), int(d["has_gauss"]), float(d["cached_gaussian"])))


def save_state(tree, path: str) -> None:
    """write `path` through `path + ".tmp"`: flush, fsync, rename.  A process killed while writing leaves the previous
    file as it was and at most a `.tmp` next to it."""
    _check_tree(tree)                    # refuse before a file is opened
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        save_tree(tree, f)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def load_state(path: str):
    with open(path, "rb") as f:
        return load_tree(f)


def state_steps(dir: str) -> List[int]:
    """the N of every `{dir}/{N}.pkl`, ascending; `.tmp` files and every other name are ignored"""
    try:
        names = os.listdir(dir)
    except (FileNotFoundError, NotADirectoryError):
        return []
    return sorted(int(nm[:-4]) for nm in names if nm.endswith(".pkl") and nm[:-4].isascii() and nm[:-4].isdigit())


def latest_state(dir: str) -> Optional[int]:
    """the largest N for which `{dir}/{N}.pkl` exists, or None"""
    steps = state_steps(dir)
    return steps[-1] if steps else None
