"""A small ordered directed graph: what grid_parser.py and kv_parser.py need of a graph library and nothing more.

The table parsers of the reference are written on a general graph library, and their RESULTS depend on the order in which
that library hands out nodes, neighbours and components (which duplicate of a split cell is numbered first, which of two key chains comes
first among equals).  The product does not import that library, so the order is restated here as a contract:

  * nodes iterate in the order they were first added (`add_node`, or implicitly by `add_edge`: u before v);
  * `successors(u)` iterates in the order the edges u -> v were first added; adding an edge that exists only updates its
    attributes and keeps its place;
  * `predecessors(v)` iterates in the order the edges u -> v were first added TO THIS OBJECT.  `copy()` re-adds the edges in
    `edges()` order (node order, then successor order), so a copy's predecessor order is by source node, not by the
    original's history - the reference's library does the same, and the row / column normalisation works on copies;
  * `edges()` iterates by source node in node order, then in successor order;
  * removing a node or an edge leaves the order of everything else alone; a node added again goes to the end;
  * `weakly_connected_components()` / `connected_components(...)` yield the components in the order of their first node;
    inside a component the members are listed in node order (the reference's library yields sets; nothing may depend on more).

tests/test_ordered_digraph.py holds the contract on hand-built graphs and, where the reference's graph library is installed,
against it on random graphs.
"""

from __future__ import annotations


class OrderedDiGraph:
    def __init__(self):
        self.nodes = {}   # node -> attribute dict, in insertion order
        self._succ = {}   # u -> {v: edge attribute dict}
        self._pred = {}   # v -> {u: the same edge attribute dict}

    # ---- construction
    def add_node(self, n, **attrs):
        if n not in self.nodes:
            self.nodes[n] = {}
            self._succ[n] = {}
            self._pred[n] = {}
        self.nodes[n].update(attrs)

    def add_nodes(self, nodes):
        for n in nodes:
            self.add_node(n)

    def add_edge(self, u, v, **attrs):
        self.add_node(u)
        self.add_node(v)
        data = self._succ[u].get(v, {})
        data.update(attrs)
        self._succ[u][v] = data
        self._pred[v][u] = data

    def remove_edge(self, u, v):
        del self._succ[u][v]
        del self._pred[v][u]

    def remove_edges(self, edges):
        for u, v in edges:
            if u in self._succ and v in self._succ[u]:
                self.remove_edge(u, v)

    def remove_node(self, n):
        for v in list(self._succ[n]):
            del self._pred[v][n]
        for u in list(self._pred[n]):
            del self._succ[u][n]
        del self.nodes[n], self._succ[n], self._pred[n]

    # ---- queries
    def __contains__(self, n):
        return n in self.nodes

    def __len__(self):
        return len(self.nodes)

    def successors(self, u):
        return list(self._succ[u])

    def predecessors(self, v):
        return list(self._pred[v])

    def edge(self, u, v):
        """The attribute dict of the edge u -> v (KeyError when there is none)."""
        return self._succ[u][v]

    def has_edge(self, u, v):
        return u in self._succ and v in self._succ[u]

    def edges(self):
        """[(u, v, attrs)]: by source in node order, then in successor order."""
        return [(u, v, d) for u, nbrs in self._succ.items() for v, d in nbrs.items()]

    def in_degree(self, n):
        return len(self._pred[n])

    def out_degree(self, n):
        return len(self._succ[n])

    # ---- derived graphs
    def copy(self):
        g = OrderedDiGraph()
        for n, attrs in self.nodes.items():
            g.add_node(n, **attrs)
        for u, v, d in self.edges():
            g.add_edge(u, v, **d)
        return g

    def edge_subgraph(self, keep, all_nodes=True):
        """The edges for which keep(attrs) holds, as a new graph.  Nodes come in the order those edges mention them; with
        `all_nodes` the remaining nodes follow in this graph's order (node attributes are not carried over)."""
        g = OrderedDiGraph()
        for u, v, d in self.edges():
            if keep(d):
                g.add_edge(u, v, **d)
        if all_nodes:
            g.add_nodes(self.nodes)
        return g

    def descendants_by(self, head, keep):
        """`head` and everything reachable from it along the edges for which keep(attrs) holds, in breadth-first order,
        each node once."""
        if head not in self.nodes:
            return []
        out, seen, at = [head], {head}, 0
        while at < len(out):
            for v, d in self._succ[out[at]].items():
                if v not in seen and keep(d):
                    seen.add(v)
                    out.append(v)
            at += 1
        return out

    # ---- components
    def weakly_connected_components(self):
        return connected_components(self.nodes, ((u, v) for u, v, _ in self.edges()))


def connected_components(nodes, edges):
    """Components of the undirected graph (nodes, edges), edges given as (u, v) pairs whose ends need not be in `nodes`
    (they are appended in the order met).  In order of their first node; members in node order."""
    order = {}
    for n in nodes:
        order.setdefault(n, len(order))
    adj = {n: [] for n in order}
    for u, v in edges:
        for n in (u, v):
            if n not in order:
                order[n] = len(order)
                adj[n] = []
        adj[u].append(v)
        adj[v].append(u)
    seen = set()
    comps = []
    for n in order:
        if n in seen:
            continue
        seen.add(n)
        comp, stack = [n], [n]
        while stack:
            for w in adj[stack.pop()]:
                if w not in seen:
                    seen.add(w)
                    comp.append(w)
                    stack.append(w)
        comps.append(sorted(comp, key=order.__getitem__))
    return comps


class UnionFind:
    """Disjoint sets over range(n) with path compression and union by size; `groups()` lists the sets in the order of their
    smallest member, members ascending."""

    def __init__(self, n):
        self.parent = list(range(n))
        self.size = [1] * n

    def find(self, x):
        root = x
        while self.parent[root] != root:
            root = self.parent[root]
        while self.parent[x] != root:
            self.parent[x], x = root, self.parent[x]
        return root

    def union(self, x, y):
        rx, ry = self.find(x), self.find(y)
        if rx == ry:
            return False
        if self.size[rx] < self.size[ry]:
            rx, ry = ry, rx
        self.parent[ry] = rx
        self.size[rx] += self.size[ry]
        return True

    def same(self, x, y):
        return self.find(x) == self.find(y)

    def group_size(self, x):
        return self.size[self.find(x)]

    def groups(self):
        out = {}
        for i in range(len(self.parent)):
            out.setdefault(self.find(i), []).append(i)
        return list(out.values())

    def group_id(self):
        ids, out = {}, []
        for i in range(len(self.parent)):
            out.append(ids.setdefault(self.find(i), len(ids)))
        return out
