"""Rolling pass: a likelihood summed over data rows as ONE term function, a table of per-row constants and a loop.

The unrolled scalar graph of ``sum_i f(theta, row_i)`` (``trace.py``) is N copies of one small expression that differ only in
constants; straight-line code for it stops at ``runtime.MAX_HMC_NODES`` live operations - about 150 rows x 6 features.  ``roll``
takes the VALUE graph (never its gradient: differentiating the unrolled graph is what takes seconds and exceeds the limit) and

  * flattens the value into signed addends (``add`` / ``sub`` / ``neg``, ``mul`` / ``div`` by a constant, carrying the coefficient;
    addends that are the same node are merged, their coefficients summed);
  * writes every addend in a canonical shape: its reachable subgraph in operand-order DFS with three kinds of leaf - the inputs
    ``th[j]``, UNIFORMS (non-leaf nodes that more than one addend reaches: hash-consing makes ``exp(th[D-1])`` of a hierarchical
    scale one id; they are cut off and numbered) and constants, which become SLOTS in first-visit order, one per occurrence, the
    carried coefficient last.  A sign in front of a sum of constant multiples is pushed into the constants (exact in IEEE
    arithmetic), so that ``log sigmoid(-z_i)`` of a row with label 0 has the shape of ``log sigmoid(z_i)`` of a row with label 1;
  * groups addends of equal shape; groups of at least ``ROLL_MIN_ROWS`` members are rolled, the ``MAX_GROUPS`` largest at most;
    everything else stays in the REST graph.  A slot with one value in every row goes back to a literal; at most ``MAX_SLOTS``
    remain per row;
  * differentiates each group's TEMPLATE (inputs: D thetas + U uniforms + S slots) in reverse mode w.r.t. its D + U non-slot
    inputs - the row loop accumulates ``lp``, ``g[D]`` and ``gu[U]`` - and the rest as ``rest(theta) + sum_k w_k u_k(theta)``
    w.r.t. theta with ``w`` as extra inputs: the uniforms' adjoints from the loop flow back through it as ``w = gu``.

Pure Python / numpy.  ``Rolled.evaluate`` is the numpy interpreter of the rolled program (next to ``ir.Graph.evaluate``): the tests and
the trace-time check against torch.autograd use it, the product path does not.
"""
from __future__ import annotations

import math

import numpy as np

from .ir import BINARY, BOOL, COMPARE, LEAVES, UNARY, Graph, Unsupported

ROLL_MIN_ROWS = 8       # a group smaller than this stays in the rest graph
MAX_GROUPS = 4          # rolled groups of one callable (the largest win)
MAX_SLOTS = 64          # per-row constants of one group that differ between rows
MAX_UNIFORMS = 32       # nodes shared between rows (functions of theta alone), evaluated once per gradient
MAX_ADDENDS = 400_000   # flattening stops here (a DAG of adds can repeat its addends)


class Group:
    """One rolled group: `template` (Graph of D + U + S inputs), its `value` node, `grads` (D + U nodes: d value / d theta and
    d value / d uniform), and `table` [rows, S] float64 (cast to the run's dtype when it is uploaded)."""

    def __init__(self, template, value, grads, table, live):
        self.template, self.value, self.grads, self.table, self.live = template, value, grads, table, live

    @property
    def rows(self):
        return self.table.shape[0]

    @property
    def slots(self):
        return self.table.shape[1]


class Rolled:
    """The rolled program of one traced callable.  `rest` is a Graph of D + U inputs (theta, then the weights w of the uniforms) that
    holds the uniforms (`u_nodes`, functions of theta), the value of everything that was not rolled (`rest_value`) and
    `rest_grads` = d (rest_value + sum_k w_k u_k) / d theta."""

    def __init__(self, D, groups, rest, u_nodes, rest_value, rest_grads, rest_live, n_addends):
        self.D, self.groups, self.rest, self.u_nodes = D, groups, rest, u_nodes
        self.rest_value, self.rest_grads, self.rest_live, self.n_addends = rest_value, rest_grads, rest_live, n_addends

    @property
    def U(self):
        return len(self.u_nodes)

    @property
    def rows(self):
        return [g.rows for g in self.groups]

    def evaluate(self, theta, dtype=None):
        """[..., 1 + D]: value and gradient of the rolled program at theta[..., D], every operation carried out in `dtype` - what
        the kernel computes, in the order it computes it up to the split of the row loop over waves."""
        theta = np.asarray(theta)
        dt = np.dtype(dtype or theta.dtype)
        lead = theta.shape[:-1]
        th = theta.reshape(-1, self.D).astype(dt)
        P, D, U = th.shape[0], self.D, self.U
        u = self.rest.evaluate(self.u_nodes, np.concatenate([th, np.zeros((P, U), dt)], axis=1), dt) if U else np.zeros((P, 0), dt)
        acc = np.zeros((P, 1 + D + U), dt)
        for gr in self.groups:
            x = np.empty((P, gr.rows, D + U + gr.slots), dt)
            x[:, :, :D] = th[:, None, :]
            x[:, :, D:D + U] = u[:, None, :]
            x[:, :, D + U:] = gr.table.astype(dt)[None]
            acc += gr.template.evaluate([gr.value] + gr.grads, x, dt).sum(axis=1, dtype=dt)
        r = self.rest.evaluate([self.rest_value] + self.rest_grads, np.concatenate([th, acc[:, 1 + D:]], axis=1), dt)
        out = acc[:, :1 + D] + r
        return out.reshape(lead + (1 + D,))


def _flatten(g, value):
    """[(coefficient, node)] with value = sum coefficient * node, merged by node, in first-visit order."""
    coef, order = {}, []
    stack = [(int(value), 1.0)]
    visits = 0
    while stack:
        n, c = stack.pop()
        visits += 1
        if visits > MAX_ADDENDS:
            raise Unsupported("the value has more than %d addends" % MAX_ADDENDS)
        nd = g.nodes[n]
        op = nd[0]
        if op == "add":
            stack.append((nd[2], c)); stack.append((nd[1], c))
            continue
        if op == "sub":
            stack.append((nd[2], -c)); stack.append((nd[1], c))
            continue
        if op == "neg":
            stack.append((nd[1], -c))
            continue
        if op == "mul":
            k, x = (nd[1], nd[2]) if g.is_const(nd[1]) else (nd[2], nd[1])
            if g.is_const(k) and math.isfinite(g.cval(k)) and math.isfinite(c * g.cval(k)) and c * g.cval(k) != 0.0:
                stack.append((x, c * g.cval(k)))
                continue
        if op == "div" and g.is_const(nd[2]):
            k = g.cval(nd[2])
            if math.isfinite(k) and k != 0.0 and math.isfinite(c / k) and c / k != 0.0:
                stack.append((nd[1], c / k))
                continue
        if n in coef:
            coef[n] += c
        else:
            coef[n] = c
            order.append(n)
    return [(coef[n], n) for n in order]


def _shared_nodes(g, addends):
    """Non-leaf nodes that more than one addend reaches (the topmost ones: the walk of a later addend stops where it meets another's)."""
    owner, shared = {}, set()
    for idx, (_, n) in enumerate(addends):
        stack = [n]
        while stack:
            i = stack.pop()
            nd = g.nodes[i]
            if nd[0] in LEAVES:
                continue
            o = owner.get(i)
            if o is None:
                owner[i] = idx
                stack.extend(nd[1:])
            elif o != idx:
                shared.add(i)
    return shared


def _canonical(g, n, shared):
    """(program, slots) of the addend node n.  program: tuple of (op, operand...) in DFS post-order; an operand is ("t", k) - the
    k-th instruction -, ("in", j), ("u", node id of a uniform), ("s", slot) or ("lit", leaf) for a boolean constant / finfo_max.
    slots: the constants in first-visit order, one per occurrence.  The last entry, ("top", operand), names the addend."""
    prog, slots, memo, push_memo = [], [], {}, {}

    def emit(*ins):
        prog.append(ins)
        return ("t", len(prog) - 1)

    def pushable(i):
        """A sign in front of node i disappears into constants below it."""
        r = push_memo.get(i)
        if r is None:
            nd = g.nodes[i]
            op = nd[0]
            if i in shared:
                r = False
            elif op in ("const", "neg"):
                r = True
            elif op in ("mul", "div"):
                r = g.is_const(nd[1]) or g.is_const(nd[2])
            elif op in ("add", "sub"):
                r = pushable(nd[1]) and pushable(nd[2])
            else:
                r = False
            push_memo[i] = r
        return r

    def ref(i, s):
        nd = g.nodes[i]
        op = nd[0]
        if op == "const":
            slots.append(s * g.cval(i))
            return ("s", len(slots) - 1)
        if op in ("bconst", "finfo_max"):
            r = ("lit", nd)
            return r if s > 0 else emit("neg", r)
        key = (i, s)
        out = memo.get(key)
        if out is not None:
            return out
        if op == "in":
            out = ("in", nd[1]) if s > 0 else emit("neg", ("in", nd[1]))
        elif i in shared:
            out = ("u", i) if s > 0 else emit("neg", ("u", i))
        elif op == "neg":
            out = ref(nd[1], -s)
        elif s < 0 and not pushable(i):
            out = emit("neg", ref(i, 1))
        elif s < 0:
            if op == "add":
                out = emit("add", ref(nd[1], -1), ref(nd[2], -1))
            elif op == "sub":
                out = emit("sub", ref(nd[2], 1), ref(nd[1], 1))
            elif g.is_const(nd[1]):
                out = emit(op, ref(nd[1], -1), ref(nd[2], 1))
            else:
                out = emit(op, ref(nd[1], 1), ref(nd[2], -1))
        else:
            out = emit(op, *[ref(x, 1) for x in nd[1:]])
        memo[key] = out
        return out

    prog.append(("top", ref(n, 1)))
    return tuple(prog), slots


def _apply(G, op, args):
    if op in UNARY:
        return G.unary(op, *args)
    if op in BINARY:
        return G.binary(op, *args)
    if op in COMPARE:
        return G.compare(op, *args)
    if op in BOOL:
        return G.boolean(op, *args)
    if op == "sel":
        return G.select(*args)
    raise Unsupported("roll: operation %r" % (op,))      # pragma: no cover


def _leaf(G, nd):
    if nd[0] == "bconst":
        return G.bconst(nd[1])
    if nd[0] == "finfo_max":
        return G.finfo_max()
    return G.const(float("nan") if nd[1] == "nan" else nd[1])


def _copy(g, roots, R):
    """Copy what `roots` depend on from graph g into graph R (inputs by index); {node of g: node of R}."""
    m = {}
    for i in g.reachable(roots):
        nd = g.nodes[i]
        if nd[0] == "in":
            m[i] = R.inputs[nd[1]]
        elif nd[0] in LEAVES:
            m[i] = _leaf(R, nd)
        else:
            m[i] = _apply(R, nd[0], [m[x] for x in nd[1:]])
    return m


def _same(col):
    return bool(np.all(col == col[0]) or np.all(np.isnan(col)))


def roll(g: Graph, value, max_nodes):
    """The rolled program of the value node `value` of graph g; raises Unsupported (no group, or a limit) with the reason.
    `max_nodes` bounds the live operations of each template (value + gradient) and of uniforms + rest."""
    D = g.n_inputs
    addends = _flatten(g, value)
    shared = _shared_nodes(g, addends)
    shapes, rest = {}, []
    for c, n in addends:
        if g.nodes[n][0] in LEAVES and g.nodes[n][0] != "in":
            rest.append((c, n))
            continue
        try:
            prog, slots = _canonical(g, n, shared)
        except RecursionError:
            rest.append((c, n))
            continue
        shapes.setdefault(prog, []).append((c, n, slots))
    ranked = sorted(shapes.items(), key=lambda kv: -len(kv[1]))          # (stable: equal sizes keep their first-visit order)
    chosen = [kv for kv in ranked if len(kv[1]) >= ROLL_MIN_ROWS][:MAX_GROUPS]
    if not chosen:
        raise Unsupported("no %d addends of the value share one shape (%d addends, the largest group has %d): nothing to roll"
                          % (ROLL_MIN_ROWS, len(addends), len(ranked[0][1]) if ranked else 0))
    taken = set(id(kv[1]) for kv in chosen)
    for prog, members in ranked:
        if id(members) not in taken:
            rest += [(c, n) for c, n, _ in members]
    uids = sorted({r[1] for prog, _ in chosen for ins in prog for r in ins[1:] if r[0] == "u"})
    U = len(uids)
    if U > MAX_UNIFORMS:
        raise Unsupported("%d nodes are shared between the rows (limit %d uniforms)" % (U, MAX_UNIFORMS))
    upos = {n: k for k, n in enumerate(uids)}

    groups = []
    for prog, members in chosen:
        full = np.array([slots + [c] for c, _, slots in members], dtype=np.float64).reshape(len(members), -1)
        vary = [k for k in range(full.shape[1]) if not _same(full[:, k])]
        if len(vary) > MAX_SLOTS:
            raise Unsupported("a row of the rolled group of %d rows has %d constants that differ between rows (limit %d slots)"
                              % (len(members), len(vary), MAX_SLOTS))
        col = {k: j for j, k in enumerate(vary)}
        T = Graph(D + U + len(vary))

        def slot(k):
            return T.inputs[D + U + col[k]] if k in col else T.const(full[0, k])

        vals = []

        def val(r):
            kind = r[0]
            if kind == "t":
                return vals[r[1]]
            if kind == "in":
                return T.inputs[r[1]]
            if kind == "u":
                return T.inputs[D + upos[r[1]]]
            if kind == "s":
                return slot(r[1])
            return _leaf(T, r[1])

        for ins in prog[:-1]:
            vals.append(_apply(T, ins[0], [val(r) for r in ins[1:]]))
        tv = T.mul(slot(full.shape[1] - 1), val(prog[-1][1]))
        grads = T.grad(tv, wrt=T.inputs[:D + U])
        live = len(T.reachable([tv] + grads))
        if live > max_nodes:
            raise Unsupported("the term of the rolled group of %d rows is %d scalar operations with its gradient (limit %d)"
                              % (len(members), live, max_nodes))
        groups.append(Group(T, tv, grads, np.ascontiguousarray(full[:, vary]), live))

    R = Graph(D + U)
    m = _copy(g, uids + [n for _, n in rest], R)
    u_nodes = [m[n] for n in uids]
    rv = R.const(0.0)
    for c, n in rest:
        rv = R.add(rv, R.mul(R.const(c), m[n]))
    F = rv
    for k in range(U):
        F = R.add(F, R.mul(R.inputs[D + k], u_nodes[k]))
    rgrads = R.grad(F, wrt=R.inputs[:D])
    rlive = len(R.reachable(u_nodes + [rv] + rgrads))
    if rlive > max_nodes:
        raise Unsupported("the uniforms and what was not rolled are %d scalar operations with their gradient (limit %d)" % (rlive, max_nodes))
    return Rolled(D, groups, R, u_nodes, rv, rgrads, rlive, len(addends))
