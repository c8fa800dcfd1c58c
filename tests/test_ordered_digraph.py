"""The order contract of yomitoku_amd.utils.graph (its module docstring): on hand-built graphs, and - where networkx is
installed - against networkx, whose iteration order the reference's table parsers rest on."""
import random

import pytest

from yomitoku_amd.utils.graph import OrderedDiGraph, UnionFind, connected_components


def _graph():
    g = OrderedDiGraph()
    g.add_node("n3", role="header")
    g.add_edge("n1", "n2", dir="R")
    g.add_edge("n3", "n2", dir="D")
    g.add_edge("n1", "n0", dir="D")
    g.add_edge("n2", "n1", dir="L")
    return g


def test_insertion_order_of_nodes_successors_predecessors_and_edges():
    g = _graph()
    assert list(g.nodes) == ["n3", "n1", "n2", "n0"] and g.nodes["n3"] == {"role": "header"} and len(g) == 4
    assert g.successors("n1") == ["n2", "n0"] and g.predecessors("n2") == ["n1", "n3"]
    assert [(u, v, d["dir"]) for u, v, d in g.edges()] == [("n3", "n2", "D"), ("n1", "n2", "R"), ("n1", "n0", "D"), ("n2", "n1", "L")]
    assert (g.in_degree("n2"), g.out_degree("n2"), g.in_degree("n3"), g.out_degree("n1")) == (2, 1, 0, 2)
    g.add_edge("n1", "n2", dir="X", w=1)  # an existing edge keeps its place; its attributes are updated
    assert g.successors("n1") == ["n2", "n0"] and g.edge("n1", "n2") == {"dir": "X", "w": 1} and g.has_edge("n1", "n2")
    g.add_node("n1", role="cell")         # so does an existing node
    assert list(g.nodes)[1] == "n1" and g.nodes["n1"] == {"role": "cell"}


def test_removal_keeps_the_order_of_the_rest_and_a_node_added_again_goes_last():
    g = _graph()
    g.remove_edge("n1", "n2")
    assert g.successors("n1") == ["n0"] and g.predecessors("n2") == ["n3"] and not g.has_edge("n1", "n2")
    g.remove_edges([("n3", "n2"), ("n9", "n2"), ("n3", "n0")])  # edges that are not there are passed over
    assert g.predecessors("n2") == []
    g = _graph()
    g.remove_node("n1")
    assert list(g.nodes) == ["n3", "n2", "n0"] and g.successors("n2") == [] and g.predecessors("n2") == ["n3"] and "n1" not in g
    g.add_edge("n1", "n3")
    assert list(g.nodes) == ["n3", "n2", "n0", "n1"]


def test_copy_orders_predecessors_by_source_node():
    g = _graph()
    g.add_edge("n0", "n2")                     # history: n1, n3, n0
    assert g.predecessors("n2") == ["n1", "n3", "n0"]
    c = g.copy()
    assert list(c.nodes) == list(g.nodes) and [e[:2] for e in c.edges()] == [e[:2] for e in g.edges()]
    assert c.predecessors("n2") == ["n3", "n1", "n0"]  # by source in node order
    c.edge("n1", "n2")["dir"] = "changed"
    c.nodes["n3"]["role"] = "cell"
    assert g.edge("n1", "n2")["dir"] == "R" and g.nodes["n3"]["role"] == "header"


def test_edge_subgraph_and_walk():
    g = _graph()
    h = g.edge_subgraph(lambda d: d.get("dir") == "D")
    assert list(h.nodes) == ["n3", "n2", "n1", "n0"] and [e[:2] for e in h.edges()] == [("n3", "n2"), ("n1", "n0")]
    assert list(g.edge_subgraph(lambda d: d.get("dir") == "R", all_nodes=False).nodes) == ["n1", "n2"]
    assert g.descendants_by("n3", lambda d: d["dir"] in ("D", "L")) == ["n3", "n2", "n1", "n0"]
    assert g.descendants_by("n1", lambda d: True) == ["n1", "n2", "n0"] and g.descendants_by("nope", lambda d: True) == []


def test_components_come_in_order_of_their_first_node():
    g = OrderedDiGraph()
    for n in "edcba":
        g.add_node(n)
    g.add_edge("a", "e")
    g.add_edge("b", "c")
    assert g.weakly_connected_components() == [["e", "a"], ["d"], ["c", "b"]]
    assert connected_components("xyz", [("z", "x"), ("q", "y")]) == [["x", "z"], ["y", "q"]]
    assert connected_components([], []) == []


def test_union_find():
    u = UnionFind(6)
    assert u.union(0, 3) and u.union(4, 3) and not u.union(0, 4) and u.union(1, 5)
    assert u.groups() == [[0, 3, 4], [1, 5], [2]] and u.group_id() == [0, 1, 2, 0, 0, 1]
    assert u.same(3, 4) and not u.same(2, 5) and u.group_size(4) == 3 and u.group_size(2) == 1


def test_against_networkx_on_random_digraphs():
    nx = pytest.importorskip("networkx", reason="networkx is not installed: the comparison with it is left out")
    rng = random.Random(20260)
    for _ in range(200):
        n = rng.randint(1, 12)
        names = [f"v{i}" for i in range(n)]
        rng.shuffle(names)
        ours, theirs = OrderedDiGraph(), nx.DiGraph()
        for name in names[: rng.randint(0, n)]:
            ours.add_node(name, k=name)
            theirs.add_node(name, k=name)
        for _ in range(rng.randint(0, 3 * n)):
            u, v = rng.choice(names), rng.choice(names)
            if u == v:
                continue
            kind = rng.choice("RLDU")
            ours.add_edge(u, v, dir=kind)
            theirs.add_edge(u, v, dir=kind)
        for _ in range(rng.randint(0, 3)):  # removals, and copies in between
            if len(ours) > 1 and rng.random() < 0.5:
                victim = rng.choice(list(ours.nodes))
                ours.remove_node(victim)
                theirs.remove_node(victim)
            elif ours.edges():
                u, v, _ = rng.choice(ours.edges())
                ours.remove_edges([(u, v)])
                theirs.remove_edges_from([(u, v)])
            if rng.random() < 0.5:
                ours, theirs = ours.copy(), theirs.copy()
        assert list(ours.nodes) == list(theirs.nodes)
        assert [(u, v, d) for u, v, d in ours.edges()] == [(u, v, d) for u, v, d in theirs.edges(data=True)]
        for node in ours.nodes:
            assert ours.successors(node) == list(theirs.successors(node)) and ours.predecessors(node) == list(theirs.predecessors(node))
            assert ours.in_degree(node) == theirs.in_degree(node) and ours.out_degree(node) == theirs.out_degree(node)
        assert [set(c) for c in ours.weakly_connected_components()] == [set(c) for c in nx.weakly_connected_components(theirs)]
        for kind in "RD":  # the edge-filtered components the grid parser takes its row / column heads from
            und = nx.Graph()
            und.add_nodes_from(theirs.nodes())
            und.add_edges_from((u, v) for u, v, d in theirs.edges(data=True) if d.get("dir") == kind)
            got = connected_components(ours.nodes, ((u, v) for u, v, d in ours.edges() if d.get("dir") == kind))
            assert [set(c) for c in got] == [set(c) for c in nx.connected_components(und)]
            sub = nx.DiGraph((u, v, d) for u, v, d in theirs.edges(data=True) if d.get("dir") == kind)
            sub.add_nodes_from(theirs.nodes())
            mine = ours.edge_subgraph(lambda d: d.get("dir") == kind)
            assert list(mine.nodes) == list(sub.nodes) and [n for n in mine.nodes if mine.in_degree(n) == 0] == [n for n in sub.nodes if sub.in_degree(n) == 0]
