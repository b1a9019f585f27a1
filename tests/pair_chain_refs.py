"""Chains and oracles shared by the pairwise-link-probability tests
(``test_pair_probabilities``, ``test_gpu_pair_counts``)."""

from collections import Counter
from itertools import combinations

import numpy as np
import pyarrow as pa

from dblink_amd.engine.writers import LinkageChainWriter

SIZE_MIX = (1, 1, 1, 2, 2, 3, 5, 17)  # RLdata-like cluster sizes, one big one


def chain_table(samples):
    """samples: [(iteration, {pid: [cluster, ...]})] -> linkage-chain table."""
    rows = {"iteration": [], "partitionId": [], "linkageStructure": []}
    for it, parts in samples:
        for pid, clusters in sorted(parts.items()):
            rows["iteration"].append(it)
            rows["partitionId"].append(pid)
            rows["linkageStructure"].append(clusters)
    return pa.table(rows, schema=LinkageChainWriter.SCHEMA)


# Ids whose string order ("10" < "9" < "B" < "a") differs from the numeric
# and from the first-appearance order; S = 4 samples over 2 partitions;
# clusters of sizes 0, 1, 2, 3. ("10", "9") is linked in all 4 samples,
# ("B", "a") in exactly 2, ("10", "a") and ("9", "a") in 1.
HAND_SAMPLES = [
    (10, {0: [["9", "10"], []], 1: [["a"], ["B"]]}),
    (20, {0: [["10", "9"]], 1: [["a", "B"]]}),
    (30, {0: [["a", "9", "10"]], 1: [["B"]]}),
    (40, {0: [["B", "a"], []], 1: [["9", "10"]]}),
]
HAND_ROWS = [("10", "9", 4), ("10", "a", 1), ("9", "a", 1), ("B", "a", 2)]


def random_samples(num_records=200, num_samples=25, seed=0):
    """Random partitions of records "0".."199" into clusters with sizes
    drawn from SIZE_MIX, each sample split over two partitions."""
    rng = np.random.default_rng(seed)
    ids = [str(i) for i in range(num_records)]
    samples = []
    for s in range(num_samples):
        perm = rng.permutation(num_records)
        clusters, at = [], 0
        while at < num_records:
            size = int(rng.choice(SIZE_MIX))
            clusters.append([ids[i] for i in perm[at:at + size]])
            at += size
        half = len(clusters) // 2
        samples.append((s + 1, {0: clusters[:half], 1: clusters[half:]}))
    return samples


def oracle_counts(samples):
    """Pure-Python oracle -> sorted [(id1, id2, count)], id1 < id2."""
    counts = Counter()
    for _, parts in samples:
        for clusters in parts.values():
            for cluster in clusters:
                for x, y in combinations(cluster, 2):
                    if x != y:
                        counts[(min(x, y), max(x, y))] += 1
    return [(x, y, c) for (x, y), c in sorted(counts.items())]


def rows_of(result):
    """pairwise_link_counts output -> [(id1, id2, count)]."""
    uniq_ids, a, b, count, _ = result
    return list(zip(uniq_ids[a].tolist(), uniq_ids[b].tolist(), count.tolist()))
