"""numpy restatement of the kept set of a sparse baked volume (include/pixelnerf_hip.h, "baked volumes", the sparse paragraph): from
a boolean array of occupied CELLS to `corner`, `keep`, `ids` and `index` over the grid POINTS, written with loops over the eight
neighbours and nothing shared with the kernel.  Point p = (i ny + j) nz + k, the order of pnr_gen_grid_points."""
import numpy as np


def corner_points(cells):
    """cells (nx-1,ny-1,nz-1) bool -> corner (nx,ny,nz) bool: a point is a corner of at least one occupied cell"""
    cells = np.asarray(cells, bool)
    nx, ny, nz = (n + 1 for n in cells.shape)
    corner = np.zeros((nx, ny, nz), bool)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                corner[di:di + nx - 1, dj:dj + ny - 1, dk:dk + nz - 1] |= cells
    return corner


def kept_points(cells):
    """-> keep (nx,ny,nz) bool: corner[p] | corner[p ^ 1] over the LINEAR ids (the pairs (2j, 2j+1) of the dense launch; with an odd
    number of points the last one has no partner)"""
    corner = corner_points(cells)
    flat = corner.reshape(-1)
    keep = flat.copy()
    for p in range(flat.size):
        q = p ^ 1
        if q < flat.size and flat[q]:
            keep[p] = True
    return keep.reshape(corner.shape)


def sparse_points(cells):
    """-> (index (nx,ny,nz) int32: the rank of a kept point among the kept ones, -1 elsewhere; ids (M,) int32 ascending)"""
    keep = kept_points(cells)
    ids = np.flatnonzero(keep.reshape(-1)).astype(np.int32)
    index = np.full(keep.size, -1, np.int32)
    index[ids] = np.arange(ids.size, dtype=np.int32)
    return index.reshape(keep.shape), ids


def occupied_cells(sigma, threshold=0.0):
    """pnr_occupancy_build at dilate 0 on a finite field: a cell any of whose 8 corners is > threshold"""
    s = np.asarray(sigma) > threshold
    nx, ny, nz = s.shape
    cells = np.zeros((nx - 1, ny - 1, nz - 1), bool)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                cells |= s[di:di + nx - 1, dj:dj + ny - 1, dk:dk + nz - 1]
    return cells


def cells_from_bits(bits, reso):
    """the words of pnr_occupancy_build -> (nx-1,ny-1,nz-1) bool"""
    shape = tuple(n - 1 for n in reso)
    n = shape[0] * shape[1] * shape[2]
    words = np.asarray(bits).astype(np.int64) & 0xFFFFFFFF
    idx = np.arange(n)
    return ((words[idx >> 5] >> (idx & 31)) & 1).astype(bool).reshape(shape)


def bits_from_cells(cells):
    """(nx-1,ny-1,nz-1) bool -> the int32 words of pnr_occupancy_build (the unused high bits of the last word zero)"""
    flat = np.asarray(cells, bool).reshape(-1)
    words = np.zeros((flat.size + 31) // 32, np.uint32)
    for c in np.flatnonzero(flat):
        words[c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    return words.view(np.int32)


def grids():
    """name -> cells of the grids the host and the GPU tests share besides the common volume: all empty, all full, the smallest
    grid, and (3,3,3) with only the last cell on (27 points: the last one has no partner)"""
    last = np.zeros((2, 2, 2), bool)
    last[1, 1, 1] = True
    return {"empty": np.zeros((4, 3, 2), bool), "full": np.ones((4, 3, 2), bool), "2x2x2": np.ones((1, 1, 1), bool), "3x3x3 last": last}
