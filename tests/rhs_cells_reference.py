"""gmg_assemble_rhs and gmg_distribute_constraints restated in plain Python loops from the arrays of
Problem.rhs_assembly_inputs() alone (include/gmg_coulomb.h has the normative text).  Python floats are IEEE doubles and
a * b + c is two roundings, so the loops below fix the same operand order and the same bits as the definition:

  1. per slot s = c nv + i:   F[s] = +0.0;  for q ascending   F[s] += ((shape[q][i] * rho[c][q]) * weight[q]) * jxw_of_level[l]
  2. then, for j ascending over the vertices of c whose line has line_inhomogeneity != 0.0:
       F[s] = F[s] - K_of_level[l][i][j] * line_inhomogeneity[line(j)]
  3. per DoF d:   rhs[d] = +0.0;  over the slots in ascending order: an unconstrained d_i == d adds F[s]; a constrained d_i adds
     line_weight[e] * F[s] for its entries e in stored order with line_master[e] == d.

Nothing here calls the host assembly, gmg_rhs_assemble or tests/rhs_reference.py."""
import numpy as np


def _lists(inp, source):
    src = inp.source if source is None else source
    return dict(
        nv=1 << int(inp.dim), nq=int(inp.nq), n_dofs=int(inp.n_dofs),
        dofs=np.asarray(inp.cell_dofs, dtype=np.int64).reshape(-1, 1 << int(inp.dim)).tolist(),
        level=np.asarray(inp.cell_level, dtype=np.int64).tolist(),
        cons=np.asarray(inp.constraint_of_dof, dtype=np.int64).tolist(),
        lp=[] if inp.line_ptr is None else np.asarray(inp.line_ptr, dtype=np.int64).tolist(),
        lm=[] if inp.line_master is None else np.asarray(inp.line_master, dtype=np.int64).tolist(),
        lw=[] if inp.line_weight is None else np.asarray(inp.line_weight, dtype=np.float64).tolist(),
        li=[] if inp.line_inhomogeneity is None else np.asarray(inp.line_inhomogeneity, dtype=np.float64).tolist(),
        K=None if inp.K_of_level is None else np.asarray(inp.K_of_level, dtype=np.float64).reshape(16, 1 << int(inp.dim), 1 << int(inp.dim)).tolist(),
        shape=np.asarray(inp.shape, dtype=np.float64).reshape(int(inp.nq), 1 << int(inp.dim)).tolist(),
        weight=np.asarray(inp.weight, dtype=np.float64).tolist(), jxw=np.asarray(inp.jxw_of_level, dtype=np.float64).tolist(),
        rho=np.asarray(src, dtype=np.float64).reshape(-1, int(inp.nq)).tolist())


def slot_values(inp, source=None):
    """F [n_cells, nv] after steps 1 and 2"""
    t = _lists(inp, source)
    nv, nq = t["nv"], t["nq"]
    F = []
    for c, dofs in enumerate(t["dofs"]):
        l = t["level"][c]
        jxw = t["jxw"][l]
        rho = t["rho"][c]
        row = []
        for i in range(nv):
            f = 0.0
            for q in range(nq):
                f += ((t["shape"][q][i] * rho[q]) * t["weight"][q]) * jxw
            for j in range(nv):
                line = t["cons"][dofs[j]]
                if line >= 0 and t["li"][line] != 0.0:
                    f = f - t["K"][l][i][j] * t["li"][line]
            row.append(f)
        F.append(row)
    return np.array(F, dtype=np.float64).reshape(len(t["dofs"]), nv)


def assemble(inp, source=None):
    """rhs [n_dofs]: steps 1 to 3.  The slots are visited once in ascending order and every rhs[d] receives its terms in that
    order, which is the per-DoF walk of the definition."""
    t = _lists(inp, source)
    F = slot_values(inp, source).tolist()
    rhs = [0.0] * t["n_dofs"]
    for c, dofs in enumerate(t["dofs"]):
        for i, d in enumerate(dofs):
            line = t["cons"][d]
            if line < 0:
                rhs[d] += F[c][i]
                continue
            for e in range(t["lp"][line], t["lp"][line + 1]):
                rhs[t["lm"][e]] += t["lw"][e] * F[c][i]
    return np.array(rhs, dtype=np.float64)


def distribute(inp, u):
    """gmg_distribute_constraints: every constrained entry from its line, read from the vector as it came in"""
    cons = np.asarray(inp.constraint_of_dof, dtype=np.int64).tolist()
    lp, lm = np.asarray(inp.line_ptr, dtype=np.int64).tolist(), np.asarray(inp.line_master, dtype=np.int64).tolist()
    lw, li = np.asarray(inp.line_weight, dtype=np.float64).tolist(), np.asarray(inp.line_inhomogeneity, dtype=np.float64).tolist()
    src = np.asarray(u, dtype=np.float64).tolist()
    out = list(src)
    for d, line in enumerate(cons):
        if line < 0:
            continue
        v = li[line]
        for e in range(lp[line], lp[line + 1]):
            v += lw[e] * src[lm[e]]
        out[d] = v
    return np.array(out, dtype=np.float64)


def masters_unconstrained(inp):
    """the precondition of gmg_distribute_constraints: no master is itself constrained"""
    cons = np.asarray(inp.constraint_of_dof)
    lm = np.asarray(inp.line_master, dtype=np.int64)
    return bool(np.all(cons[lm] < 0)) if lm.size else True


def features(inp):
    """what a mesh holds for the comparison: (hanging-node lines, cells with a nonzero Dirichlet term, cells with both a
    hanging node and a nonzero Dirichlet term, DoFs that are master of more than one line)"""
    cons = np.asarray(inp.constraint_of_dof, dtype=np.int64)
    n_ent = np.diff(np.asarray(inp.line_ptr, dtype=np.int64))
    li = np.asarray(inp.line_inhomogeneity, dtype=np.float64)
    cd = np.asarray(inp.cell_dofs, dtype=np.int64)
    line = cons[cd]
    has = line >= 0
    safe = np.maximum(line, 0)
    hang = has & (n_ent[safe] > 0) if len(n_ent) else np.zeros_like(has)
    inhom = has & (li[safe] != 0.0) if len(li) else np.zeros_like(has)
    lm = np.asarray(inp.line_master, dtype=np.int64)
    owner = np.repeat(np.arange(len(n_ent)), n_ent)
    pairs = np.unique(np.stack([lm, owner], axis=1), axis=0) if lm.size else np.zeros((0, 2), dtype=np.int64)
    multi = int(np.sum(np.bincount(pairs[:, 0], minlength=1) > 1)) if len(pairs) else 0
    return (int(np.sum(n_ent > 0)), int(np.sum(np.any(inhom, axis=1))), int(np.sum(np.any(inhom, axis=1) & np.any(hang, axis=1))), multi)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
