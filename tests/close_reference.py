"""Boundary values and constraints.close() restated over lists and Python floats: the definition of gmg_close_constraints
(include/gmg_coulomb.h).  Input: the UNCLOSED tables (constraint_of_dof, line_ptr, line_master,
line_weight, n_hanging, n_lines) and one value per Dirichlet line; output: the closed CSR and the inhomogeneities.  A Python
float is an IEEE double and `w * v` then `s + p` round twice, which is what the definition asks for (no fused multiply-add)."""
from types import SimpleNamespace


class HangingMaster(Exception):
    """a hanging node constrained to a hanging node"""


def close(constraint_of_dof, line_ptr, line_master, line_weight, n_hanging, n_lines, dirichlet_value=None):
    """namespace(line_ptr, line_master, line_weight, line_inhomogeneity) of the closed lines.  dirichlet_value None: all +0.0."""
    H, L = int(n_hanging), int(n_lines)
    if dirichlet_value is None:
        dirichlet_value = [0.0] * (L - H)
    if len(dirichlet_value) != L - H:
        raise ValueError("one value per Dirichlet line")
    inhom = [0.0] * H + [float(v) for v in dirichlet_value]
    ptr, master, weight = [0], [], []
    for l in range(L):
        if l >= H and line_ptr[l + 1] != line_ptr[l]:
            raise ValueError("a Dirichlet line with entries")
        for e in range(line_ptr[l], line_ptr[l + 1]):
            m = constraint_of_dof[line_master[e]]
            if m < 0:
                master.append(int(line_master[e]))
                weight.append(float(line_weight[e]))
            elif m >= H:
                product = float(line_weight[e]) * inhom[m]
                inhom[l] = inhom[l] + product
            else:
                raise HangingMaster(f"line {l}: master {line_master[e]} has the hanging line {m}")
        ptr.append(len(master))
    return SimpleNamespace(line_ptr=ptr, line_master=master, line_weight=weight, line_inhomogeneity=inhom)


def close_tables(t, dirichlet_value=None):
    """close() of anything that carries the unclosed tables as attributes (mesh_tables_reference.build, Context.get_mesh_tables)"""
    return close(list(t.constraint_of_dof), list(t.line_ptr), list(t.line_master), list(t.line_weight), t.n_hanging, t.n_lines, dirichlet_value)
