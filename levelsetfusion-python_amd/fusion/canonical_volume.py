"""CanonicalVolume: the weighted canonical TSDF on the device, with its fusion, ray-cast, mesh, shift and brick calls
(the package's docstring has the rules)."""
import math

import numpy as np
import torch

from .. import (device_esdf, device_fusion, device_mesh, device_mesh_components, device_mesh_simplify,
                device_mesh_smooth, device_raycast, device_volume_bricks, device_volume_shift)
from ..device_core import require_gpu
from ..rigid_opt.frame_tracker import device_colour_image
from ..tsdf.generation import device_depth, offsets_of
from .brick_store import BrickStore


def _model_shape(shape):
    s = (int(shape),) * 3 if np.ndim(shape) == 0 else tuple(int(v) for v in shape)
    if len(s) not in (2, 3) or min(s) < 1:
        raise ValueError("a canonical volume has two or three extents >= 1, got %s" % (s,))
    return s


def _live(live):
    if isinstance(live, torch.Tensor):
        return live if live.is_cuda else live.to("cuda")
    a = np.asarray(live)
    if a.dtype.kind not in "fiub":
        raise ValueError("live must be numeric, got %s" % a.dtype)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")


def _on_device(x, name, dtype, move=True):
    """x, a numpy array of `dtype` or a tensor, as a device tensor.  move=False leaves a tensor where it is: a CPU
    tensor is then refused by the device check of the call, not moved"""
    if isinstance(x, torch.Tensor):
        return x.to("cuda") if move and not x.is_cuda else x
    a = np.asarray(x)
    if a.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, np.dtype(dtype).name, a.dtype))
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def simplified(out, normals, colours, simplify_cell):
    """device_mesh.extract_mesh's tuple clustered by the lattice of edge simplify_cell through the origin (None: as it
    is), with the normals and colours that were asked for, and the record or None"""
    if simplify_cell is None:
        return out, None
    v, f, n, c, record = device_mesh_simplify.simplify(out[0], out[1], out[2] if normals else None,
                                                       out[3] if colours else None, simplify_cell)
    return ((v, f, n, c) if colours else (v, f, n)), record


def components_filtered(out, normals, colours, min_component_faces, keep_largest_components):
    """device_mesh.extract_mesh's tuple without the components of fewer than min_component_faces faces, and of the rest
    only the keep_largest_components largest (both None: as it is), with the normals and colours that were asked for,
    and the record or None"""
    if min_component_faces is None and keep_largest_components is None:
        return out, None
    v, f, n, c, record = device_mesh_components.filter(out[0], out[1], out[2] if normals else None,
                                                       out[3] if colours else None, min_faces=min_component_faces,
                                                       keep_largest=keep_largest_components)
    return ((v, f, n, c) if colours else (v, f, n)), record


def smoothed(out, normals, colours, smooth_iterations, smooth_boundary):
    """device_mesh.extract_mesh's tuple after smooth_iterations Taubin iterations with the default lambda and mu (None:
    as it is), its normals rebuilt from the smoothed faces when they were asked for, and the record or None"""
    if smooth_iterations is None:
        return out, None
    v, f, n, c, record = device_mesh_smooth.smooth(out[0], out[1], out[2] if normals else None,
                                                   out[3] if colours else None, smooth_iterations,
                                                   boundary=smooth_boundary)
    return ((v, f, n, c) if colours else (v, f, n)), record


def mesh_outputs(out, normals, colours, as_tensor=False):
    """of device_mesh.extract_mesh's (vertices, faces, normals[, colours]) the ones asked for, in that order: the
    device tensors with as_tensor, numpy copies otherwise"""
    kept = tuple(t for t, keep in zip(out, (True, True, normals, colours)) if keep)
    return kept if as_tensor else tuple(t.cpu().numpy() for t in kept)


class CanonicalVolume:
    """the weighted canonical TSDF: `tsdf` and `weight`, float32 device tensors of `shape` ((Z, Y, X), (H, W) or an
    int for a cube).  Depth mode needs a 3-D volume.  With colour=True (3-D only) also `colour`, a float32 device
    tensor of shape (Z, Y, X, 4): R, G, B in 0..255 and the colour weight, all 0 at the start; None otherwise."""

    def __init__(self, shape, max_weight=math.inf, colour=False):
        if colour and np.ndim(shape) != 0 and np.size(shape) != 3:
            raise ValueError("a colour volume needs a 3-D model, got shape %s" % (tuple(shape),))
        require_gpu()
        self.shape = _model_shape(shape)
        device_fusion.fusion_weights(1.0, max_weight)
        self.max_weight = max_weight
        self.tsdf = torch.ones(self.shape, dtype=torch.float32, device="cuda")
        self.weight = torch.zeros(self.shape, dtype=torch.float32, device="cuda")
        self.colour = torch.zeros(self.shape + (4,), dtype=torch.float32, device="cuda") if colour else None
        self._spare = None  # shift: the buffers the next shifted copy is written to
        self._bricks = None  # shift(brick_store=): the flags, offsets and total of the brick count, kept like _spare
        self.mesh_record = None  # extract_mesh(simplify_cell=): the last simplification's record
        self._esdf = None  # esdf: the scratch volumes and the record's buffer, kept like _spare
        self.last_esdf_record = None  # esdf: the last call's record
        self.last_esdf_offset = None  # esdf(brick_store=): the array offset of the box the last field covers

    def reset(self):
        """back to the empty model: tsdf 1, weight 0 everywhere (and a colour volume 0)"""
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        if self.colour is not None:
            self.colour.zero_()

    def integrate_volume(self, live, weight=1.0):
        """fuse a live field of the model's shape (numpy or a float32 device tensor); returns the device record"""
        return device_fusion.integrate_volume(self.tsdf, self.weight, _live(live), weight, self.max_weight)

    def integrate_depth(self, depth_image, camera, twist, array_offset, voxel_size=0.004, narrow_band_width_voxels=20,
                        weight=1.0, pixel_weight=None, carve=False, colour_image=None, colour_band=1.0, warp=None):
        """generate the live volume of depth_image (uint16 / float32 / float64, numpy or device) under twist, as the
        rigid tracker does, and fuse it in the same pass; returns the device record.  pixel_weight (a float32 image of
        depth_image's shape, numpy or device) and carve choose the weighted rule (package docstring), whose record
        unpack_weighted_record reads; with neither the call is the unweighted one.  colour_image (uint8 (H, W, 3),
        numpy or device, registered to depth_image; the volume must have been made with colour=True) also fuses colour
        inside (-colour_band, colour_band), the geometry as the weighted rule does; unpack_colour_record reads its
        record.  warp (float32, the model's shape + (3,), numpy or device: x, y, z displacement in voxels, what
        HierarchicalOptimizer3d.optimize(model, live) returns) makes every voxel observe the frame at its displaced
        point, by the weighted rule and with colour_image the colour rule (package docstring); unpack_warped_record
        reads its record of nine doubles.  Without a warp nothing changes."""
        depth, code = device_depth(depth_image)
        if colour_image is not None and self.colour is None:
            raise ValueError("colour_image needs a volume made with colour=True")
        if pixel_weight is not None:
            pixel_weight = _on_device(pixel_weight, "pixel_weight", np.float32, move=False)
        if colour_image is not None:
            colour_image = device_colour_image(colour_image)
        if warp is not None:
            warp = _on_device(warp, "warp", np.float32)
        return device_fusion.integrate_depth_by_arguments(
            self.tsdf, self.weight, depth, code, camera, array_offset, twist, voxel_size, narrow_band_width_voxels,
            weight, self.max_weight, pixel_weight, carve, self.colour, colour_image, colour_band, warp)[0]

    def raycast(self, camera, twist, array_offset, voxel_size=0.004, image_shape=(480, 640), normals=False,
                fallback_depth=None, as_tensor=False, colours=False):
        """the model seen from a pinhole camera at twist (the generator's convention: twist_vector_to_matrix3d of the
        float32-rounded twist maps world to camera): float32 depth (H, W) in metres, 0 where a ray hits nothing, and
        with normals=True the unit normals (H, W, 3) in camera coordinates.  fallback_depth (uint16 / float32 /
        float64, numpy or device, scaled by camera.depth_unit_ratio) fills the pixels without a hit.  Returns depth or
        (depth, normals): device tensors with as_tensor=True, enqueued without waiting; numpy copies otherwise.  With
        colours=True (a volume made with colour=True) the float32 (H, W, 4) image of (R, G, B, Y) at the hit points is
        appended -- R, G, B in units of the 8-bit image, Y = (0.299 R + 0.587 G + 0.114 B) / 255, four NaNs where a
        pixel has no hit or its hit point no colour -- and the result is always a tuple."""
        fb, code = (None, None) if fallback_depth is None else device_depth(fallback_depth)
        if colours and self.colour is None:
            raise ValueError("colours=True needs a volume made with colour=True")
        cast = device_raycast.raycast(self.tsdf, self.weight, camera, twist, array_offset, voxel_size, image_shape,
                                      normals, fb, code, colour=self.colour if colours else None)
        out = (cast[0], cast[1]) if normals else (cast[0],)
        if colours:
            out += (cast[3],)
        if not as_tensor:
            out = tuple(t.cpu().numpy() for t in out)
        return out if normals or colours else out[0]

    def extract_mesh(self, array_offset, voxel_size=0.004, iso=0.0, min_weight=0.0, normals=False, as_tensor=False,
                     colours=False, default_colour=device_mesh.DEFAULT_COLOUR, simplify_cell=None,
                     min_component_faces=None, keep_largest_components=None, smooth_iterations=None,
                     smooth_boundary="fixed"):
        """the level set iso of the model as a triangle mesh, with raycast's conventions (voxel (i, j, k) at
        ((k, j, i) + array_offset) * voxel_size): float32 vertices (V, 3) in world metres, (x, y, z); int32 faces
        (F, 3), their right-hand normal towards larger tsdf; with normals=True also the float32 unit normals (V, 3).
        Only cells whose 8 corners have weight > min_weight draw.  Returns (vertices, faces) or (vertices, faces,
        normals): device tensors with as_tensor=True, numpy copies otherwise.  With colours=True (a volume made with
        colour=True) the uint8 vertex colours (V, 3) are appended, row i the colour of vertex i, default_colour where
        neither end of the vertex's grid edge has a colour.  One host synchronisation: the read of the two totals.
        simplify_cell (metres) passes the mesh through vertex clustering on the lattice of that edge through the world
        origin before it is returned -- simplify_mesh(extract_mesh(...), simplify_cell) without the copies -- for one
        more host synchronisation, the read of its record, which `mesh_record` keeps.
        min_component_faces and keep_largest_components remove floaters last, after simplify_cell:
        filter_mesh_components(mesh, min_faces=min_component_faces, keep_largest=keep_largest_components) without the
        copies, for two more host synchronisations; `mesh_record` then is a dict that holds the simplification's fields,
        if that ran, and the components' record under "components".  With both None the call and `mesh_record` are as
        they were.
        smooth_iterations runs that many Taubin iterations after simplify_cell and before the component filter, which
        stays last: smooth_mesh(mesh, smooth_iterations, boundary=smooth_boundary) with the default lambda and mu and
        without the copies, the normals rebuilt from the smoothed faces with normals=True, for one more host
        synchronisation; `mesh_record` then is such a dict with the smoothing's record under "smooth".  With None the
        call, its launches and `mesh_record` are as they were."""
        if len(self.shape) != 3:
            raise ValueError("mesh extraction needs a 3-D model, this one has shape %s" % (self.shape,))
        if colours and self.colour is None:
            raise ValueError("colours=True needs a volume made with colour=True")
        out = device_mesh.extract_mesh(self.tsdf, self.weight, array_offset, voxel_size, iso, min_weight, normals,
                                       *((self.colour, default_colour) if colours else ()))
        out, self.mesh_record = simplified(out, normals, colours, simplify_cell)
        out, record = smoothed(out, normals, colours, smooth_iterations, smooth_boundary)
        if record is not None:
            self.mesh_record = dict(self.mesh_record or {}, smooth=record)
        out, record = components_filtered(out, normals, colours, min_component_faces, keep_largest_components)
        if record is not None:
            self.mesh_record = dict(self.mesh_record or {}, components=record)
        return mesh_outputs(out, normals, colours, as_tensor)

    def esdf(self, voxel_size=0.004, max_distance_voxels=32, iso=0.0, min_weight=0.0, unknown="free", nearest=False,
             as_tensor=False, brick_store=None, array_offset=None, max_voxels=2 ** 28):
        """the Euclidean signed distance field of the model (package docstring, "Euclidean distance field"): float32
        (Z, Y, X) in metres, the distance from each voxel's centre to the centre of the nearest site -- an observed
        voxel (weight > min_weight) with an observed 6-neighbour on the other side of iso -- negative where the voxel
        itself is observed with tsdf < iso, and +-max_distance_voxels * voxel_size where no site lies within
        max_distance_voxels (1 .. 4096; the cap is inclusive).  unknown="free" leaves voxels that were never observed
        out of the sites: they carry a positive distance like free space, and `weight` masks them if the caller wants
        that; unknown="occupied" makes every one of them a site.  With nearest=True returns (esdf, nearest), nearest the
        int32 flat index (z Y + y) X + x of that site, the smallest among equally near ones, -1 beyond the cap.
        Device tensors with as_tensor=True, numpy copies otherwise.  `last_esdf_record` keeps {"sites", "finite",
        "max_distance2"}: the sites, the voxels within the cap and the largest squared lattice distance among them.
        One host synchronisation: the read of that record.  With brick_store and the window's array_offset the field
        is that of `assemble(brick_store, array_offset, max_voxels)`, window and store, over the lattice box of the
        two, whose array offset `last_esdf_offset` keeps (None otherwise); assemble's refusals apply."""
        if len(self.shape) != 3:
            raise ValueError("a distance field needs a 3-D model, this one has shape %s" % (self.shape,))
        if (brick_store is None) != (array_offset is None):
            raise ValueError("brick_store and array_offset go together: the store's lattice is placed by the window's "
                             "array_offset")
        device_esdf.params(self.shape, voxel_size, max_distance_voxels, iso, min_weight, unknown)  # before any device work
        tsdf, weight, worker, self.last_esdf_offset = self.tsdf, self.weight, self._esdf, None
        if brick_store is not None:
            tsdf, weight, _, self.last_esdf_offset = self.assemble(brick_store, array_offset, max_voxels)
            worker = device_esdf.Esdf()  # the box is another shape: its scratch does not outlive the call
        elif worker is None:
            worker = self._esdf = device_esdf.Esdf()
        field, _, site, self.last_esdf_record = worker.compute(tsdf, weight, voxel_size, max_distance_voxels, iso,
                                                               min_weight, unknown)
        out = (field, site) if nearest else (field,)
        if not as_tensor:
            out = tuple(t.cpu().numpy() for t in out)
        return out if nearest else out[0]

    def _leaving_mesh(self, box, array_offset, voxel_size, min_weight, normals, colours):
        """the host mesh of one box of leaving cells ((x0, x1), (y0, y1), (z0, z1)): extract_mesh of a contiguous copy
        of its voxels -- the cells' range plus one layer on the high side -- with array_offset moved by its origin"""
        (x0, x1), (y0, y1), (z0, z1) = box
        part = (slice(z0, z1 + 1), slice(y0, y1 + 1), slice(x0, x1 + 1))
        colour = self.colour[part].contiguous() if colours else None
        out = device_mesh.extract_mesh(self.tsdf[part].contiguous(), self.weight[part].contiguous(),
                                       offsets_of(array_offset) + np.array([x0, y0, z0], dtype=np.float64),
                                       voxel_size, 0.0, min_weight, normals, colour)
        return mesh_outputs(out, normals, colours)

    def _brick_lattice(self, brick_store, array_offset, fix=True):
        """the window's lattice origin g in `brick_store` after the checks that need no device"""
        if not isinstance(brick_store, BrickStore):
            raise ValueError("brick_store must be a fusion.BrickStore or None, got %r" % (brick_store,))
        if len(self.shape) != 3:
            raise ValueError("a brick store needs a 3-D model, this one has shape %s" % (self.shape,))
        if brick_store.colour != (self.colour is not None):
            raise ValueError("the brick store was made with colour=%r, the volume with colour=%r: they must agree"
                             % (brick_store.colour, self.colour is not None))
        return brick_store.lattice_origin(array_offset, fix)

    def _bricks_out(self, store, g, s):
        """steps 2-4 of a shift with a store: count, the one host read, gather, the rows' copy to the host, the merge"""
        B = device_volume_bricks
        if self._bricks is None:  # the largest grid any alignment of this shape has
            most = int(np.prod([(n + B.BRICK - 2) // B.BRICK + 1 for n in self.shape]))
            self._bricks = (torch.empty(most, dtype=torch.int32, device=self.tsdf.device),
                            torch.empty(most, dtype=torch.int32, device=self.tsdf.device),
                            torch.empty(1, dtype=torch.int64, device=self.tsdf.device))
        nbricks = int(np.prod(B.brick_grid(self.shape, g)[1]))
        flags, offsets, total = self._bricks[0][:nbricks], self._bricks[1][:nbricks], self._bricks[2]
        B.count(self.weight, flags, offsets, total, g, s)
        k = int(total.item())  # the host wait of a shift with a store
        if k == 0:
            return 0, 0
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=self.tsdf.device)
        cube = (k, B.BRICK, B.BRICK, B.BRICK)
        rows = (new((k, 3), torch.int32), new(cube, torch.float32), new(cube, torch.float32),
                None if self.colour is None else new(cube + (4,), torch.float32), new((k, B.VALID_BYTES), torch.uint8))
        B.gather(self.tsdf, self.weight, self.colour, flags, offsets, k, *rows, g, s)
        return k, store.merge(*(None if t is None else t.cpu().numpy() for t in rows))

    def _bricks_in(self, store, g, s):
        """steps 6-8: the stored bricks that touch what entered a window at lattice origin g under s go up, are
        scattered into the window's buffers and lose the validity bits of what was written"""
        B = device_volume_bricks
        coords, tsdf, weight, colour, valid = store.lookup_entering(*B.entering_flags(self.shape, g, s))
        taken = B.entering_mask(self.shape, g, s, coords) & B.unpack_valid(valid)
        touched = taken.reshape(len(coords), B.BRICK_VOXELS).any(axis=1)
        if not touched.any():
            return 0, 0
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a[touched])).to(self.tsdf.device)
        B.scatter(up(coords), up(tsdf), up(weight), up(colour), up(valid), self.tsdf, self.weight, self.colour, g, s)
        store.clear_valid(coords[touched], taken[touched])
        return int(touched.sum()), int(taken.sum())

    def assemble(self, brick_store, array_offset, max_voxels=2 ** 28):
        """the whole map, window and store, as fresh dense device tensors over the lattice bounding box of the two:
        (tsdf, weight, colour or None, array_offset_of_box).  The box is filled with the empty voxel, the window is
        copied in, and one lsf_volume_bricks_scatter with an all-entering shift writes the stored voxels; a stored
        voxel inside the window is never valid, so the order does not matter.  array_offset is the window's.
        ValueError when the box has more than max_voxels voxels, or more than 2^31 - 1."""
        g = np.array(self._brick_lattice(brick_store, array_offset, fix=False), dtype=np.int64)
        n = np.array(self.shape[::-1], dtype=np.int64)
        lo, hi = g, g + n
        bounds = brick_store.bounds()
        if bounds is not None:
            lo, hi = np.minimum(lo, bounds[0]), np.maximum(hi, bounds[1])
        dims = hi - lo
        voxels = int(dims[0]) * int(dims[1]) * int(dims[2])
        if voxels > min(int(max_voxels), 0x7fffffff):
            raise ValueError("the map's box has %d x %d x %d voxels (x, y, z), more than max_voxels = %d or than "
                             "int32 indices reach" % (dims[0], dims[1], dims[2], max_voxels))
        shape = tuple(int(v) for v in dims[::-1])
        tsdf = torch.ones(shape, dtype=torch.float32, device=self.tsdf.device)
        weight = torch.zeros(shape, dtype=torch.float32, device=self.tsdf.device)
        colour = None if self.colour is None else torch.zeros(shape + (4,), dtype=torch.float32,
                                                              device=self.tsdf.device)
        x0, y0, z0 = (int(v) for v in g - lo)
        part = (slice(z0, z0 + self.shape[0]), slice(y0, y0 + self.shape[1]), slice(x0, x0 + self.shape[2]))
        tsdf[part], weight[part] = self.tsdf, self.weight
        if colour is not None:
            colour[part] = self.colour
        if len(brick_store):
            rows = brick_store.lookup(brick_store.coords())
            up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.tsdf.device)
            device_volume_bricks.scatter(*(up(a) for a in rows), tsdf, weight, colour, tuple(int(v) for v in lo),
                                         (shape[2], 0, 0))
        return tsdf, weight, colour, offsets_of(array_offset) + (lo - g).astype(np.float64)

    def shift(self, shift_voxels, array_offset, voxel_size=0.004, stream_mesh=False, min_weight=0.0, normals=False,
              colours=False, brick_store=None):
        """move the window by shift_voxels = (sx, sy, sz) whole voxels: afterwards voxel v holds what voxel v + s held,
        and the voxels that entered are empty (tsdf 1, weight 0, colour 0); one launch of csrc/lsf_volume_shift.hip.
        Returns (new_array_offset, chunks) with new_array_offset = array_offset + s (float64 (3,)), under which every
        retained voxel keeps its world point bit for bit.  3-D volumes only.  The copy is out of place into a spare
        set of buffers, allocated at the first non-zero shift, and `tsdf`, `weight` and `colour` are swapped with
        them: no later call allocates, and a tensor taken from these attributes BEFORE a shift is the spare
        afterwards (the next shift overwrites it).  A zero shift returns (array_offset, []) at once, without a launch.
        With stream_mesh the cells that leave -- a cell, the cube between voxel c and c + 1, leaves when any of its 8
        corners does -- are meshed first, at iso 0 with extract_mesh's kernels: device_volume_shift.leaving_boxes cuts
        them into at most three disjoint boxes, each meshed from a contiguous copy of its voxels, and `chunks` lists
        their host tuples in extract_mesh's layout (with normals / colours as asked; boxes without a face are left
        out).  Every cell of the old volume is thus drawn exactly once across the chunks and the new window; the
        seam's vertices appear in both, nothing is welded.  Each box costs extract_mesh's host read.
        With brick_store (a BrickStore whose `colour` matches the volume's) the window is lossless: the first such
        call fixes the store's lattice at array_offset, and every later array_offset must lie whole voxels from it.
        In order: the bricks holding a voxel that leaves with data are counted (lsf_volume_bricks_count) and the total
        is read on the host; those bricks are gathered and copied to the host; the store merges them (valid voxels
        overwrite, validity bits are ORed); the shifted copy runs as above; the store's bricks that touch what entered
        are uploaded and scattered into the new buffers; the store clears the validity bits of what was written and
        drops the bricks left without one.  A voxel that leaves without data is not kept and comes back empty.
        `brick_store.last` has the counts.  The return value is unchanged.  Cost: one host wait for the total and the
        copies of the rows, both ways; the workspaces of the count are allocated once per volume."""
        if len(self.shape) != 3:
            raise ValueError("a volume shift needs a 3-D model, this one has shape %s" % (self.shape,))
        s = device_volume_shift.shift_of(shift_voxels)
        offset = offsets_of(array_offset).copy()
        if colours and self.colour is None:
            raise ValueError("colours=True needs a volume made with colour=True")
        g = None if brick_store is None else self._brick_lattice(brick_store, offset)
        if brick_store is not None:
            brick_store.last = {"bricks_out": 0, "voxels_out": 0, "bricks_in": 0, "voxels_in": 0}
        if s == (0, 0, 0):
            return offset, []
        chunks = []
        if stream_mesh:
            for box in device_volume_shift.leaving_boxes(self.shape, s):
                mesh = self._leaving_mesh(box, offset, voxel_size, min_weight, normals, colours)
                if len(mesh[1]):
                    chunks.append(mesh)
        if self._spare is None:
            self._spare = (torch.empty_like(self.tsdf), torch.empty_like(self.weight),
                           None if self.colour is None else torch.empty_like(self.colour))
        out_tsdf, out_weight, out_colour = self._spare
        if brick_store is not None:
            device_volume_bricks.params(self.shape, tuple(a + b for a, b in zip(g, s)), s)  # the new origin fits too
            bricks_out, voxels_out = self._bricks_out(brick_store, g, s)
        device_volume_shift.shift(self.tsdf, self.weight, self.colour, out_tsdf, out_weight, out_colour, s)
        self._spare = (self.tsdf, self.weight, self.colour)
        self.tsdf, self.weight, self.colour = out_tsdf, out_weight, out_colour
        if brick_store is not None:
            bricks_in, voxels_in = self._bricks_in(brick_store, tuple(a + b for a, b in zip(g, s)), s)
            brick_store.last = {"bricks_out": bricks_out, "voxels_out": voxels_out, "bricks_in": bricks_in,
                                "voxels_in": voxels_in}
        return offset + np.array(s, dtype=np.float64), chunks
