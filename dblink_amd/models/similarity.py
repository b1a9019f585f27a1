"""Attribute similarity functions.

Semantics match the reference (``SimilarityFn.scala:25-107``):

- ``ConstantSimilarityFn``: similarity 0 everywhere.
- ``LevenshteinSimilarityFn(threshold, maxSimilarity)``: truncated, scaled
  normalized Levenshtein similarity (Yujian-Bo normalized metric)::

      unit(a,b)  = 1 - 2*d / (|a| + |b| + d)          (1.0 when both empty)
      sim(a,b)   = max(0, t * (S_max * unit(a,b) - thr)),  t = S_max/(S_max-thr)

- ``DamerauLevenshteinSimilarityFn(threshold, maxSimilarity)``: the same with
  ``d`` the restricted Damerau-Levenshtein (optimal string alignment)
  distance, which counts an adjacent swap as one edit. Not in the reference.
- ``JaroSimilarityFn(threshold, maxSimilarity, prefixScale)``: the same
  truncation and scaling over the Jaro similarity with the Winkler prefix
  boost (``jaro_winkler``) as ``unit``. Not in the reference.

These host implementations are the *oracle*; the batched V x V domain sweep
used to build the attribute index runs in the native extension
(CPU C++ / HIP for gfx950) — see ``dblink_amd.ops``.
"""

from __future__ import annotations


class SimilarityFn:
    is_constant = False
    # which native sweep metric (``dblink_amd.ops.sim_pairs``) computes this
    # function: "levenshtein", "osa", "jaro", or None for the pure-Python pass
    native_metric = None

    def similarity(self, a: str, b: str) -> float:
        raise NotImplementedError

    def mk_string(self) -> str:
        raise NotImplementedError


class ConstantSimilarityFn(SimilarityFn):
    is_constant = True
    threshold = 0.0
    max_similarity = 0.0

    def similarity(self, a: str, b: str) -> float:
        return 0.0

    def mk_string(self) -> str:
        return "ConstantSimilarityFn"

    def __eq__(self, other):
        return isinstance(other, ConstantSimilarityFn)

    def __hash__(self):
        return hash("ConstantSimilarityFn")


def levenshtein(a: str, b: str) -> int:
    """Plain dynamic-programming edit distance (insert/delete/substitute = 1)."""
    la, lb = len(a), len(b)
    if la == 0:
        return lb
    if lb == 0:
        return la
    prev = list(range(lb + 1))
    cur = [0] * (lb + 1)
    for i in range(1, la + 1):
        cur[0] = i
        ca = a[i - 1]
        for j in range(1, lb + 1):
            cost = 0 if ca == b[j - 1] else 1
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + cost)
        prev, cur = cur, prev
    return prev[lb]


def osa_distance(a: str, b: str) -> int:
    """Restricted Damerau-Levenshtein (optimal string alignment) distance.

    The Levenshtein recurrence plus one term: swapping two adjacent
    characters costs 1, and no substring is edited twice. It is therefore
    not the unrestricted Damerau distance: ``osa("ca", "abc") == 3`` where
    unrestricted Damerau gives 2 (swap, then insert between the swapped pair).
    """
    la, lb = len(a), len(b)
    if la == 0:
        return lb
    if lb == 0:
        return la
    prev2 = None
    prev = list(range(lb + 1))
    for i in range(1, la + 1):
        cur = [i] + [0] * lb
        ca = a[i - 1]
        for j in range(1, lb + 1):
            cost = 0 if ca == b[j - 1] else 1
            m = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + cost)
            if i > 1 and j > 1 and ca == b[j - 2] and a[i - 2] == b[j - 1]:
                m = min(m, prev2[j - 2] + 1)
            cur[j] = m
        prev2, prev = prev, cur
    return prev[lb]


def jaro_parts(a: str, b: str):
    """``(m, t)`` of the Jaro similarity: matches and transpositions.

    Window ``r = max(max(|a|, |b|) // 2 - 1, 0)``. Greedy: each ``a[i]`` in
    order takes the first unmatched ``j`` in ``[i-r, i+r]`` with
    ``b[j] == a[i]``. ``t`` is half the number of positions at which the
    matched characters of ``a`` and of ``b``, each in its own order, differ.
    """
    la, lb = len(a), len(b)
    r = max(max(la, lb) // 2 - 1, 0)
    taken = [False] * lb
    matched_a = []
    for i, ch in enumerate(a):
        for j in range(max(i - r, 0), min(i + r + 1, lb)):
            if not taken[j] and b[j] == ch:
                taken[j] = True
                matched_a.append(ch)
                break
    matched_b = [b[j] for j in range(lb) if taken[j]]
    half = sum(1 for x, y in zip(matched_a, matched_b) if x != y)
    return len(matched_a), half // 2


def jaro_boost_gate(m: int, t: int, la: int, lb: int) -> bool:
    """``jaro > 0.7`` decided in exact integers (needs ``m > 0``)."""
    return 10 * (m * m * (la + lb) + (m - t) * la * lb) > 21 * m * la * lb


def jaro(a: str, b: str) -> float:
    """Jaro similarity in [0, 1]; 1.0 when both strings are empty."""
    la, lb = len(a), len(b)
    if la == 0 and lb == 0:
        return 1.0
    m, t = jaro_parts(a, b)
    if m == 0:
        return 0.0
    return (m / la + m / lb + (m - t) / m) / 3.0


def jaro_winkler(a: str, b: str, prefix_scale: float = 0.1) -> float:
    """Jaro similarity with the Winkler boost ``l * p * (1 - jaro)`` for a
    common prefix of ``l <= 4`` characters, applied only when ``jaro > 0.7``
    (``jaro_boost_gate``)."""
    la, lb = len(a), len(b)
    if la == 0 and lb == 0:
        return 1.0
    m, t = jaro_parts(a, b)
    if m == 0:
        return 0.0
    j = (m / la + m / lb + (m - t) / m) / 3.0
    if not jaro_boost_gate(m, t, la, lb):
        return j
    l = 0
    while l < min(4, la, lb) and a[l] == b[l]:
        l += 1
    return j + l * prefix_scale * (1.0 - j)


class _ScaledSimilarityFn(SimilarityFn):
    """Truncated, scaled similarity over a unit similarity in [0, 1]::

        sim(a,b) = max(0, t * (S_max * unit(a,b) - thr)),  t = S_max/(S_max-thr)

    Subclasses define ``unit_similarity``.
    """

    is_constant = False

    def __init__(self, threshold: float = 7.0, max_similarity: float = 10.0):
        if max_similarity <= 0.0:
            raise ValueError("`maxSimilarity` must be positive")
        if not (0.0 <= threshold < max_similarity):
            raise ValueError("`threshold` must be in [0, maxSimilarity)")
        self.threshold = float(threshold)
        self.max_similarity = float(max_similarity)
        self.trans_factor = max_similarity / (max_similarity - threshold)

    def unit_similarity(self, a: str, b: str) -> float:
        raise NotImplementedError

    def similarity(self, a: str, b: str) -> float:
        s = self.trans_factor * (self.max_similarity * self.unit_similarity(a, b) - self.threshold)
        return s if s > 0.0 else 0.0


class _EditSimilarityFn(_ScaledSimilarityFn):
    """Truncated, scaled normalized similarity over an integer edit distance.

    Subclasses set ``_distance`` (the metric), ``_name`` (the config name)
    and ``native_metric``.
    """

    _distance = None
    _name = None

    def unit_similarity(self, a: str, b: str) -> float:
        total = len(a) + len(b)
        if total == 0:
            return 1.0
        d = type(self)._distance(a, b)
        return 1.0 - 2.0 * d / (total + d)

    def mk_string(self) -> str:
        return f"{self._name}(threshold={self.threshold}, maxSimilarity={self.max_similarity})"

    def __eq__(self, other):
        return (
            type(other) is type(self)
            and other.threshold == self.threshold
            and other.max_similarity == self.max_similarity
        )

    def __hash__(self):
        return hash((self._name, self.threshold, self.max_similarity))


class LevenshteinSimilarityFn(_EditSimilarityFn):
    native_metric = "levenshtein"
    _distance = staticmethod(levenshtein)
    _name = "LevenshteinSimilarityFn"


class DamerauLevenshteinSimilarityFn(_EditSimilarityFn):
    """``LevenshteinSimilarityFn`` with adjacent transpositions at cost 1.

    This is the *restricted* Damerau-Levenshtein distance (optimal string
    alignment, ``osa_distance``): "jonh"/"john" is 1 edit, not 2, but no
    substring is edited twice, so ``osa("ca", "abc") == 3`` where the
    unrestricted Damerau distance is 2.
    """

    native_metric = "osa"
    _distance = staticmethod(osa_distance)
    _name = "DamerauLevenshteinSimilarityFn"


class JaroSimilarityFn(_ScaledSimilarityFn):
    """Truncated, scaled Jaro similarity with the Winkler prefix boost.

    ``unit`` is ``jaro_winkler(a, b, prefix_scale)``; ``prefix_scale = 0``
    gives plain Jaro. The config name is ``JaroSimilarityFn``: the boost is a
    parameter (``prefixScale``), not part of the name.
    """

    native_metric = "jaro"
    _name = "JaroSimilarityFn"

    def __init__(self, threshold: float = 7.0, max_similarity: float = 10.0,
                 prefix_scale: float = 0.1):
        super().__init__(threshold, max_similarity)
        if not (0.0 <= prefix_scale <= 0.25):
            raise ValueError("`prefixScale` must be in [0, 0.25]")
        self.prefix_scale = float(prefix_scale)

    def unit_similarity(self, a: str, b: str) -> float:
        return jaro_winkler(a, b, self.prefix_scale)

    def mk_string(self) -> str:
        return (f"{self._name}(threshold={self.threshold}, "
                f"maxSimilarity={self.max_similarity}, prefixScale={self.prefix_scale})")

    def __eq__(self, other):
        return (
            type(other) is type(self)
            and other.threshold == self.threshold
            and other.max_similarity == self.max_similarity
            and other.prefix_scale == self.prefix_scale
        )

    def __hash__(self):
        return hash((self._name, self.threshold, self.max_similarity, self.prefix_scale))


_EDIT_FNS = {c._name: c for c in (LevenshteinSimilarityFn, DamerauLevenshteinSimilarityFn)}


def similarity_fn_from_config(cfg) -> SimilarityFn:
    """Build a similarity function from a config object (``Project.scala:203-217``)."""
    name = cfg.get_string("name")
    if name == "ConstantSimilarityFn":
        return ConstantSimilarityFn()
    if name in _EDIT_FNS:
        return _EDIT_FNS[name](
            threshold=cfg.get_double("parameters.threshold"),
            max_similarity=cfg.get_double("parameters.maxSimilarity"),
        )
    if name == JaroSimilarityFn._name:
        return JaroSimilarityFn(
            threshold=cfg.get_double("parameters.threshold"),
            max_similarity=cfg.get_double("parameters.maxSimilarity"),
            prefix_scale=float(cfg.get_or("parameters.prefixScale", 0.1)),
        )
    raise ValueError(f"unsupported similarity function: {name!r}")
