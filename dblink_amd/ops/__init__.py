"""Native-op dispatch layer.

Loads the in-tree native extension ``dblink_amd._C`` (C++/OpenMP host paths +
HIP gfx950 device kernels, built by ``setup.py build_ext --inplace`` or
``__graft_entry__.build()``).

Policy:
- on CPU, pure-Python/numpy fallbacks are allowed (used by tests as oracles
  and when the extension has not been built yet);
- on GPU (CUDA/HIP tensors), the native extension is REQUIRED — ops raise
  rather than silently falling back to an eager path.
"""

from __future__ import annotations

import os

import numpy as np

_C = None
_C_ERR = None
try:  # torch must be imported first so the extension can link against it
    import torch  # noqa: F401
    from dblink_amd import _C as _C  # type: ignore
except Exception as e:  # pragma: no cover - exercised only without built ext
    _C = None
    _C_ERR = e


def have_native() -> bool:
    return _C is not None


def native():
    if _C is None:
        raise RuntimeError(
            f"dblink_amd._C native extension is required but not available: {_C_ERR}\n"
            "Build it with `python setup.py build_ext --inplace`."
        )
    return _C


SIM_GPU_MAX_LEN = 256  # sim_pairs_kernel, jaro_pairs_kernel: four 64-bit words per pattern
SIM_MAX_SYMBOLS = 65535  # 16-bit symbol ids, 0 reserved for padding


def sim_pairs_route(num_values, max_len, num_symbols, cuda_available):
    """Which pass builds a domain's similarity index: ``"gpu"``, ``"cpu"``
    (native OpenMP) or ``"python"`` (pure-Python oracle).

    The GPU sweep takes domains above ``DBLINK_SIM_GPU_MIN_V`` values
    (default 8192; below it the launch and transfer overhead outweighs the
    CPU pass) whose longest value fits ``SIM_GPU_MAX_LEN`` characters. Both
    native sweeps need the alphabet to fit ``SIM_MAX_SYMBOLS`` ids.
    """
    if num_symbols > SIM_MAX_SYMBOLS:
        return "python"
    min_v = int(os.environ.get("DBLINK_SIM_GPU_MIN_V", "8192"))
    if cuda_available and num_values > min_v and max_len <= SIM_GPU_MAX_LEN:
        return "gpu"
    return "cpu"


# Pair occurrences from which the pair-count hash table is taken without
# being asked for: the smallest measured shape (10^4 records x 100 samples,
# 4.7M pair occurrences), where the table already beats the numpy arm
# 116-fold (BENCH.md, "Pairwise link counts"); nothing smaller was measured.
PAIRS_GPU_MIN_DEFAULT = 1 << 22


def have_pair_table() -> bool:
    return _C is not None and hasattr(_C, "pair_table_add")


def pair_counts_route(total_pairs, cuda_available):
    """Which arm counts the chain's co-clustered pairs: ``"gpu"`` (the
    pair-count hash table, ``pair_counts.hip``) or ``"numpy"``.

    The GPU arm takes chains of at least ``DBLINK_PAIRS_GPU_MIN`` pair
    occurrences when a device is available and the extension has the
    kernels; everything else goes to the numpy reference arm.
    """
    min_pairs = int(os.environ.get("DBLINK_PAIRS_GPU_MIN", str(PAIRS_GPU_MIN_DEFAULT)))
    if cuda_available and have_pair_table() and total_pairs >= min_pairs:
        return "gpu"
    return "numpy"


from .pair_table import PairCountTable  # noqa: E402,F401
from .cluster_table import ClusterCountTable  # noqa: E402,F401


def sim_pairs(values, similarity_fn):
    """Build the sparse exp-similarity index over a domain of strings.

    Returns a ``SimIndexCSR``. Replaces the reference's Spark ``cartesian``
    V x V sweep (``AttributeIndex.scala:219-231``) with a length-pruned
    banded edit-distance pass. ``similarity_fn.native_metric`` selects the
    metric of the native sweeps: ``"levenshtein"``, ``"osa"`` (adjacent
    transpositions at cost 1) or ``"jaro"`` (Jaro similarity with the Winkler
    prefix boost, scaled by ``similarity_fn.prefix_scale``).
    """
    from ..models.attribute_index import SimIndexCSR, _python_sim_pairs

    if similarity_fn.is_constant:
        n = len(values)
        return SimIndexCSR(np.zeros(n + 1, dtype=np.int64), np.empty(0, np.int32), np.empty(0))

    # Only a function that names a native metric may take a native sweep;
    # any other non-constant function is scored by its own similarity().
    metric = getattr(similarity_fn, "native_metric", None)
    if metric is None:
        return _python_sim_pairs(values, similarity_fn)
    if metric not in ("levenshtein", "osa", "jaro"):
        raise ValueError(f"unknown native similarity metric: {metric!r}")
    # (sweep name, last argument) of the metric's native entry points
    if metric == "jaro":
        sweep, sweep_arg = "jaro_pairs", float(similarity_fn.prefix_scale)
    else:
        sweep, sweep_arg = "sim_pairs", metric == "osa"

    # The similarity must be over CHARACTERS (the reference uses JVM strings,
    # SimilarityFn.scala:92-98). Encode through a per-domain character
    # vocabulary, one symbol id per character (0 pads), so symbol-level
    # distance == character-level: uint8 ids up to 255 distinct
    # characters, 16-bit ids (int16 storage) up to 65535.
    charset = sorted({ch for v in values for ch in v})
    lens = np.array([len(v) for v in values], dtype=np.int32)
    maxlen = int(lens.max()) if len(lens) else 0
    cuda = False
    if _C is not None and hasattr(_C, sweep + "_gpu"):
        import torch

        cuda = torch.cuda.is_available()
    route = sim_pairs_route(len(values), maxlen, len(charset), cuda)
    if route == "python" and len(charset) > SIM_MAX_SYMBOLS:
        import logging

        logging.getLogger("dblink_amd.ops").warning(
            "attribute domain has %d distinct characters (> %d): the native "
            "similarity sweeps cannot encode it; running the quadratic "
            "pure-Python pass",
            len(charset), SIM_MAX_SYMBOLS,
        )
    if route != "python" and _C is not None and hasattr(_C, sweep + "_cpu"):
        import torch

        vocab = {ch: i + 1 for i, ch in enumerate(charset)}
        wide = len(charset) > 255
        # the GPU kernel's row stride: a multiple of 64 symbols (one Myers word)
        stride = -(-max(maxlen, 1) // 64) * 64 if route == "gpu" else max(maxlen, 1)
        buf = np.zeros((len(values), stride), dtype=np.uint16 if wide else np.uint8)
        for i, v in enumerate(values):
            buf[i, : len(v)] = [vocab[ch] for ch in v]
        if wide:
            buf = buf.view(np.int16)

        thr = float(similarity_fn.threshold)
        msim = float(similarity_fn.max_similarity)
        # Large domains: run the V x V sweep on the GPU (the reference's Spark
        # cartesian analog, AttributeIndex.scala:222-231) — the quadratic pair
        # filter is the startup bottleneck at V ~ 10^5.
        if route == "gpu":
            row_ptr, col, expsim = getattr(_C, sweep + "_gpu")(
                torch.from_numpy(buf).cuda(), torch.from_numpy(lens).cuda(), thr, msim,
                sweep_arg,
            )
            # atomically-filled rows are unordered; sort within rows by col
            V = len(values)
            counts = row_ptr[1:] - row_ptr[:-1]
            row_of = torch.repeat_interleave(
                torch.arange(V, device=col.device, dtype=torch.int64), counts
            )
            keys = row_of * V + col.to(torch.int64)
            order = torch.argsort(keys)
            return SimIndexCSR(
                row_ptr.cpu().numpy(),
                col[order].cpu().numpy(),
                expsim[order].cpu().numpy().astype(np.float64),
            )
        row_ptr, col, expsim = getattr(_C, sweep + "_cpu")(
            torch.from_numpy(buf), torch.from_numpy(lens), thr, msim, sweep_arg
        )
        return SimIndexCSR(row_ptr.numpy().astype(np.int64), col.numpy(), expsim.numpy())

    return _python_sim_pairs(values, similarity_fn)
