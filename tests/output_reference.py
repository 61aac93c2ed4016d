"""What tests/test_output_cpu.py and tests/test_gpu_output.py hold the graphical output against: a numpy
restatement of the patch arrays from (cell_dofs, cell_level, vertex_of_dof, origin, h0, u), written from the definitions in
include/gmg_coulomb.h (gmg_output_patches) and not from the kernel, and a reader of the .vtu / .pvtu files made of xml.etree,
base64 and numpy alone.

Definitions.  One patch per active cell a with nv = 2^dim vertices, slot s = a nv + v, v = bx + 2 by + 4 bz, k =
vertex_of_dof[cell_dofs[s]]:
  point[s][d]    = origin + (h0 / 4096.0) * float((k >> 21 d) & 0x1fffff)   for d < dim, +0.0 above
  solution[s]    = U[v] = u[cell_dofs[a nv + v]]
  grad_phi[s][d] = -((U[v | 1 << d] - U[v & ~(1 << d)]) / (h0 / float(1 << level[a])))   for d < dim, +0.0 above
  field_j[s]     = f_j[cell_dofs[s]]
numpy forms a product, then a sum, each rounded to fp64: no fused multiply-add."""
import base64
import os
import xml.etree.ElementTree as ET
from types import SimpleNamespace

import numpy as np

HEX_ORDER = (0, 1, 3, 2, 4, 5, 7, 6)
VTK_TYPES = {"Float64": np.float64, "Float32": np.float32, "Int32": np.int32, "UInt8": np.uint8, "UInt64": np.uint64}


def patches(dim, cell_dofs, cell_level, vertex_of_dof, origin, h0, u, fields=()):
    """namespace(point [n_slots, 3], solution [n_slots], grad_phi [n_slots, 3], fields [one [n_slots] per field])"""
    nv = 1 << dim
    cd = np.asarray(cell_dofs, dtype=np.int64).reshape(-1, nv)
    lv = np.asarray(cell_level, dtype=np.int64).reshape(-1)
    keys = np.asarray(vertex_of_dof, dtype=np.uint64)
    u = np.asarray(u, dtype=np.float64)
    nc = len(cd)
    assert len(lv) == nc and len(u) == len(keys)
    origin, h0 = np.float64(origin), np.float64(h0)
    hf = h0 / np.float64(4096.0)
    k = keys[cd]
    point, grad = np.zeros((nc, nv, 3)), np.zeros((nc, nv, 3))
    U = u[cd]
    h = (h0 / np.left_shift(1, lv).astype(np.float64)).reshape(nc, 1)
    v = np.arange(nv)
    for d in range(dim):
        lattice = np.bitwise_and(np.right_shift(k, np.uint64(21 * d)), np.uint64(0x1FFFFF)).astype(np.float64)
        point[:, :, d] = origin + hf * lattice
        g = (U[:, v | (1 << d)] - U[:, v & ~(1 << d)]) / h
        grad[:, :, d] = -g
    return SimpleNamespace(point=point.reshape(-1, 3), solution=U.reshape(-1).copy(), grad_phi=grad.reshape(-1, 3),
                           fields=[np.asarray(f, dtype=np.float64)[cd].reshape(-1) for f in fields])


def connectivity(dim, n_cells):
    """(connectivity, offsets, types) of n_cells patches"""
    nv = 1 << dim
    order = np.asarray(HEX_ORDER[:nv], dtype=np.int32)
    conn = (np.arange(n_cells, dtype=np.int32)[:, None] * nv + order[None, :]).reshape(-1)
    return conn, (np.arange(n_cells, dtype=np.int32) + 1) * nv, np.full(n_cells, 12 if dim == 3 else 9, dtype=np.uint8)


def bits(a):
    """the bit patterns of an fp64 / fp32 array (so that -0.0 and +0.0 differ)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _decode(node):
    """a DataArray with format="binary": a UInt64 byte count and the bytes in one base64 run"""
    assert node.get("format") == "binary", node.attrib
    raw = base64.b64decode(node.text.strip(), validate=True)
    count = int(np.frombuffer(raw[:8], dtype="<u8")[0])
    assert count == len(raw) - 8, (node.attrib, count, len(raw))
    a = np.frombuffer(raw[8:], dtype=np.dtype(VTK_TYPES[node.get("type")]).newbyteorder("<"))
    nc = int(node.get("NumberOfComponents", "1"))
    return a.reshape(-1, nc) if nc > 1 else a


def read_vtu(path):
    """namespace(n_points, n_cells, points [n, 3], connectivity, offsets, types, point_data {name: array} in file order,
    point_types {name: VTK type}, cell_data names)"""
    root = ET.parse(path).getroot()
    assert root.tag == "VTKFile" and root.get("type") == "UnstructuredGrid" and root.get("version") == "1.0", root.attrib
    assert root.get("byte_order") == "LittleEndian" and root.get("header_type") == "UInt64", root.attrib
    assert root.get("compressor") is None
    (grid,) = list(root)
    assert grid.tag == "UnstructuredGrid"
    (piece,) = list(grid)
    (points,) = piece.find("Points")
    assert points.get("type") == "Float64" and points.get("NumberOfComponents") == "3"
    cells = {n.get("Name"): n for n in piece.find("Cells")}
    assert [n.get("Name") for n in piece.find("Cells")] == ["connectivity", "offsets", "types"]
    assert cells["connectivity"].get("type") == "Int32" and cells["offsets"].get("type") == "Int32" and cells["types"].get("type") == "UInt8"
    data, types = {}, {}
    for n in piece.find("PointData"):
        assert n.tag == "DataArray"
        data[n.get("Name")], types[n.get("Name")] = _decode(n), (n.get("type"), int(n.get("NumberOfComponents", "1")))
    cd = piece.find("CellData")
    return SimpleNamespace(n_points=int(piece.get("NumberOfPoints")), n_cells=int(piece.get("NumberOfCells")), points=_decode(points),
                           connectivity=_decode(cells["connectivity"]), offsets=_decode(cells["offsets"]), types=_decode(cells["types"]),
                           point_data=data, point_types=types, cell_data=[] if cd is None else [n.get("Name") for n in cd])


def read_pvtu(path):
    """namespace(points (type, components), point_types {name: (type, components)} in file order, pieces [Source])"""
    root = ET.parse(path).getroot()
    assert root.tag == "VTKFile" and root.get("type") == "PUnstructuredGrid" and root.get("version") == "1.0", root.attrib
    assert root.get("byte_order") == "LittleEndian" and root.get("header_type") == "UInt64", root.attrib
    (grid,) = list(root)
    assert grid.tag == "PUnstructuredGrid"
    (pp,) = grid.find("PPoints")
    types = {n.get("Name"): (n.get("type"), int(n.get("NumberOfComponents", "1"))) for n in grid.find("PPointData")}
    return SimpleNamespace(points=(pp.get("type"), int(pp.get("NumberOfComponents", "1"))), point_types=types,
                           pieces=[n.get("Source") for n in grid.findall("Piece")])


def names(cycle):
    """(piece, pvtu, visit) file names of a cycle"""
    stem = "solution-%05d" % cycle
    return stem + ".0000.vtu", stem + ".pvtu", stem + ".visit"


def read_bytes(directory, cycle):
    """the bytes of the three files of a cycle"""
    out = []
    for n in names(cycle):
        with open(os.path.join(directory, n), "rb") as f:
            out.append(f.read())
    return out
