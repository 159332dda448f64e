"""
Small numeric utilities (reference ``src/mdhelper/algorithm/utility.py``).
Only ``get_closest_factors`` (:15-72) touches the hot path (spherical wavevector
surfaces of ``StructureFactor``, reference analysis/structure.py:1383).
``find_connected_nodes`` / ``depth_first_search`` (:158-210) are host helpers for
graphs a user builds by hand; ``analysis.Clusters`` finds the clusters of a
trajectory on the GPU.
"""

from __future__ import annotations

from typing import Any

import numpy as np


def get_closest_factors(value: int, n_factors: int, reverse: bool = False) -> np.ndarray:
    """
    ``n_factors`` integers whose product is ``value`` and which lie as close to
    each other as possible, ascending (descending when ``reverse``).

    The reference walks the prime factors greedily (sympy); here the
    factorisation with the smallest spread (then the smallest sum) is found by an
    exhaustive search over divisors, which gives the same answers on the
    reference's test vectors (1000 → 10·10·10, 35904 → 32·33·34,
    73440 → 15·16·17·18) without the sympy dependency.
    """
    value, n_factors = int(value), int(n_factors)
    if value < 1 or n_factors < 1:
        raise ValueError("value and n_factors must be positive.")
    best = None

    def search(remaining, k, lowest, chosen):
        nonlocal best
        if k == 1:
            if remaining >= lowest:
                cand = chosen + [remaining]
                key = (cand[-1] - cand[0], sum(cand))
                if best is None or key < best[0]:
                    best = (key, cand)
            return
        d = lowest
        while d ** k <= remaining:
            if remaining % d == 0:
                search(remaining // d, k - 1, d, chosen + [d])
            d += 1

    search(value, n_factors, 1, [])
    factors = np.array(best[1], dtype=int)
    return factors[::-1] if reverse else factors


def depth_first_search(graph: dict[Any, list[Any]], start: Any, visited: dict[Any, bool],
                       group: list[Any]) -> None:
    """
    Appends to ``group`` every node of ``graph`` (``{node: [neighbors]}``) that can be reached from ``start``
    without passing a node already marked in ``visited``, in depth-first preorder, and marks them; ``visited`` and
    ``group`` are updated in place.

    Iterative, with an explicit stack of neighbor iterators: the order is that of the reference's recursive search,
    and a chain of any length is walked without touching Python's recursion limit.
    """
    visited[start] = True
    group.append(start)
    stack = [iter(graph[start])]
    while stack:
        for neighbor in stack[-1]:
            if not visited[neighbor]:
                visited[neighbor] = True
                group.append(neighbor)
                stack.append(iter(graph[neighbor]))
                break
        else:
            stack.pop()


def find_connected_nodes(graph: dict[Any, list[Any]]) -> list[list[Any]]:
    """
    Connected components of ``graph`` (``{node: [neighbors]}``, every neighbor a key): a list of lists of nodes,
    the components in the order of their first node in ``graph``, the nodes of one in depth-first preorder.
    """
    visited = {node: False for node in graph}
    results = []
    for start in graph:
        if not visited[start]:
            group = []
            depth_first_search(graph, start, visited, group)
            results.append(group)
    return results
