"""Refit from device arrays: the numpy float64 restatement of the library's vertex-normal rule (compute_normals,
csrc/prt_host.cpp; what prt_refit_meshes_device computes on the device for a mesh given without normals) and of the order
it sums in.  Shared by test_refit_device_host.py (against prt.Mesh without normals) and test_gpu_refit_device.py.

The rule: per face e1 = b - a, e2 = c - a and e1 x e2 in double, every product and difference rounded on its own; per
vertex the double sum over its incident corners in ascending face order, a face's repeated vertex once per corner;
l = sqrt(x x + y y + z z), n = float32(sum / l), and (0, 1, 0) where l is not > 0.  numpy's float64 element-wise
operations, sqrt and division round correctly and never fuse, so the statements below are the rule itself."""
import numpy as np


def corner_csr(indices, n_vertices):
    """(start [n_vertices + 1], corner [3 n_triangles]): vertex v's incident corners (3 * face + k) are
    corner[start[v] : start[v + 1]], ascending."""
    flat = np.asarray(indices, np.int64).reshape(-1)
    corner = np.argsort(flat, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n_vertices))])
    return start.astype(np.int64), corner.astype(np.int64)


def face_normals(vertices, indices):
    """[n_triangles, 3] float64: e1 x e2 of every face, unnormalised (twice its area)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    i = np.asarray(indices, np.int64).reshape(-1, 3)
    a, b, c = v[i[:, 0]], v[i[:, 1]], v[i[:, 2]]
    e1, e2 = b - a, c - a
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                     e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)


def vertex_normals(vertices, indices):
    """[n_vertices, 3] float32 by the rule above."""
    nv = np.asarray(vertices).reshape(-1, 3).shape[0]
    fn = face_normals(vertices, indices)
    start, corner = corner_csr(indices, nv)
    deg = np.diff(start)
    acc = np.zeros((nv, 3))
    for j in range(int(deg.max()) if nv else 0):   # round j adds every vertex's j-th incident corner: its own order is kept
        vs = np.nonzero(deg > j)[0]
        acc[vs] = acc[vs] + fn[corner[start[vs] + j] // 3]
    l = np.sqrt(acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1] + acc[:, 2] * acc[:, 2])
    ok = l > 0.0
    out = np.zeros((nv, 3), np.float32)
    out[:, 1] = 1.0
    out[ok] = (acc[ok] / l[ok, None]).astype(np.float32)
    return out


def degenerate_mesh():
    """12 vertices, 7 faces: a zero-area face (collinear corners that are in no other face), a face with a repeated
    vertex, an unreferenced vertex (11), around four ordinary faces.  Vertices 6, 7, 8 and 11 get (0, 1, 0)."""
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [0.0, 1.0, 0.2], [1.0, 1.0, -0.3], [2.0, 0.5, 0.7], [0.5, 2.0, 0.25],
                  [3.0, 0.0, 0.0], [4.0, 0.0, 0.0], [3.5, 0.0, 0.0], [2.0, 2.0, 1.0], [2.5, 1.5, -1.0], [9.0, 9.0, 9.0]], np.float32)
    i = np.array([[0, 1, 2], [1, 3, 2], [1, 4, 3], [2, 3, 5],
                  [6, 7, 8],     # zero area
                  [9, 9, 10],    # a repeated vertex
                  [3, 4, 9]], np.uint32)
    return v, i
