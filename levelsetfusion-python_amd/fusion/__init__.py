"""Fusion of tracked depth frames into a canonical TSDF volume: the model update of KillingFusion / SobolevFusion, which
the reference does not have.  INTEGRATION.md section 3 ("Fusion") defines the rule; tests/fusion_restatement.py
restates it in numpy.

CanonicalVolume holds the model, two float32 device arrays of one shape: `tsdf` (starts at 1) and `weight` (starts at
0).  A frame's live value l at a voxel is fused when -1 < l < 1, strictly:
    W1 = W + w,  tsdf = (W t + w l) / W1,  weight = min(W1, max_weight)
in float32, the average taken with the uncapped W1; every other voxel keeps its tsdf and weight bit for bit.  Each
integrate_* call is two launches of csrc/lsf_fusion.hip and returns the call's record as a float64 device tensor
(unpack_record turns a host copy into {fused, first_seen, sum_abs_change, max_abs_change}); nothing waits for the GPU.

Depth mode also has a weighted rule with free-space carving ("Weighted fusion and carving";
tests/fusion_weighted_restatement.py restates it): CanonicalVolume.integrate_depth(..., pixel_weight=, carve=).  A
voxel has a valid pixel when it lies in front of the camera, projects into the image and the depth there is > 0.  With
one it is in band when -1 < l < 1 and, with carve, carved when l == 1 exactly: the camera has looked through it, and
+1 is fused.  Its weight is w_eff = w * pixel_weight[iy][ix], one float32 multiply (w itself without an image); a
w_eff that is not finite and > 0 leaves the voxel alone and is counted.  The average then runs with w_eff in place
of w.  A surface that later frames look through is thereby averaged towards +1: a fused value t0 > -1 gives
(t0 + 1) / 2 > 0 after one carving frame of equal weight.  The record gains carved and weight_rejected
(unpack_weighted_record).  With both arguments at their defaults the call is the unweighted one, unchanged.
DepthConfidence builds the weight image c = |n . r| min(1, (reference_depth / z)^2) on the device from the level-0
depth and normals of a DepthPyramid (csrc/lsf_depth_confidence.hip; INTEGRATION.md section 3, "Depth confidence"):
grazing and far pixels, whose axial noise grows with z^2, count less.
Colour ("Colour fusion"; tests/colour_restatement.py restates it): CanonicalVolume(shape,
max_weight, colour=True) also holds `colour`, a float32 (Z, Y, X, 4) device tensor of one 16-byte record per voxel --
R, G, B in units of the 8-bit image and the colour weight Wc, all starting at 0.  integrate_depth(..., colour_image=,
colour_band=1.0) takes a uint8 (H, W, 3) image registered to the depth camera, fuses the geometry exactly as the
weighted rule does with the same arguments, and colours every voxel with a valid pixel whose live value lies strictly
inside (-colour_band, colour_band) and whose w_eff is finite and > 0:
    Wc1 = Wc + w_eff,  C_j = (Wc C_j + w_eff c_j) / Wc1,  Wc = min(Wc1, max_weight)
in float32, c_j the pixel's channel.  Carved voxels are never coloured; every other voxel keeps its record bit for bit.
A small colour_band keeps the colour of a voxel to the frames that see the surface near it, not through it.  The record
gains coloured and first_coloured (unpack_colour_record).  extract_mesh(..., colours=True) adds the uint8 (V, 3) vertex
colours: a vertex on the edge from voxel v to w takes C_v (1 - t) + C_w t with the vertex's own t when both have
Wc > 0, the colour of the one that has, else default_colour; mesh_io.write_ply(..., colours=) writes them.
CanonicalVolume.raycast renders the model into a depth (and normal) image seen from a camera at a twist: one launch of
csrc/lsf_raycast.hip ("Ray-casting"; tests/raycast_restatement.py restates it).
CanonicalVolume.extract_mesh takes the model's surface out as a triangle mesh: marching cubes over the cells whose 8
corners have weight > min_weight, with a generated case table whose meshes are watertight, in a fixed output order
("Mesh extraction"; tests/mesh_restatement.py restates it).  It is five launches of
csrc/lsf_mesh.hip with one host read of the vertex and face totals between the counting and the emitting launches;
mesh_io.write_ply writes the result.  SequenceFusion3d.extract_mesh passes the sequence's array_offset and voxel_size.

SequenceFusion3d runs a depth sequence.  Frame 0 is fused under `initial_twist` (zero by default).  Every later frame is
first tracked, started from the previous frame's twist, as `tracking_reference` chooses: by the 6-DoF rigid tracker
(device_rigid.rigid_run_3d, `rigid_iterations` iterations; 0 keeps the previous twist) against a reference volume, or
by ICP against the model's prediction:
    "model"    the model's tsdf itself (the default)
    "raycast"  the live volume, under the previous twist, of the model ray-cast at the previous twist with the holes
               filled from the previous frame's depth -- KillingFusion-style tracking against the model's prediction.
               Voxels behind the fused band keep the model's initial +1, where a frame has -1; tracking against the
               model itself meets that residual at every band's back edge, and the prediction does not have it.
    "icp"      projective point-to-plane ICP (rigid_opt.ProjectiveIcp3d, device_icp.icp_run) of the frame against the
               model ray-cast with normals at the previous twist, without a fallback image; `icp_iterations`,
               `icp_strides` and `icp_max_distance` set the pyramid, and `rigid_iterations` is not used.  With
               `icp_pyramid` (a rigid_opt.DepthPyramid) the frame's filtered depth pyramid is built on the device and
               `icp_iterations` runs over its levels (device_icp.icp_run_pyramid), `icp_strides` not used;
               `icp_max_normal_angle` (radians) adds the normal-angle gate.  Fusion still integrates the raw depth.
    "sdf"      point-to-SDF tracking (rigid_opt.PointToSdf3d, device_point_sdf.point_sdf_run; INTEGRATION.md section 3,
               "Point-to-SDF tracking"; tests/point_sdf_restatement.py restates it) of the frame's points against the
               model's tsdf and weight themselves: no prediction is ray-cast, `prediction_hits` is None, and
               `sdf_tracker` (a PointToSdf3d, PointToSdf3d(camera) by default) sets the levels, the gate and the
               loss.  `rigid_iterations` and the `icp_*` settings are not used, and `photometric_weight`,
               `icp_robust`, `icp_pyramid`, `icp_max_normal_angle` and `icp_intensity_pyramid` are refused: they belong
               to the "icp" tracker, which has a prediction image to pair into.  The tracker's own settings do the
               same here: PointToSdf3d(pyramid=) tracks on the frame's filtered depth pyramid, built once per frame
               (`confidence` shares it under "icp" mode's rule; fusion still integrates the raw depth), and
               PointToSdf3d(photometric_weight=) adds a colour term against the model's colour volume (it needs
               colour=True; with a pyramid also intensity_pyramid=), which holds the pose on a flat textured wall
               (tests/point_sdf_colour_restatement.py restates both; profiles/point_sdf_colour_cost.md).
Without a non-rigid optimizer the frame is then fused in depth mode under its twist: one launch pair, no live volume.
With `carve` or `confidence` (a DepthConfidence) every frame, frame 0 included, is fused by the weighted rule; the
confidence image comes from the frame's own pyramid -- the tracker's, built once, when "icp" mode has an `icp_pyramid`
with the filter settings of `confidence.pyramid`, else a one-level pyramid of those settings.
With `colour` the model holds a colour volume, integrate(depth_image, colour_image) needs a colour image on every frame
and fuses it through the colour entry point, with `carve` and `confidence` as set, in every tracking mode; tracking
does not read the colour unless `photometric_weight` is set.
With `photometric_weight` (lambda; it needs colour=True and tracking_reference="icp", and with an `icp_pyramid` also
an `icp_intensity_pyramid`) frames
k >= 1 are tracked by the joint geometric and photometric solve ("Photometric ICP";
rigid_opt.ProjectiveIcp3d, device_icp.icp_run_photometric; tests/photometric_restatement.py restates it) against the
model ray-cast with normals and colour at the previous twist (CanonicalVolume.raycast(..., colours=True),
lsf_raycast_colour: (R, G, B, Y) trilinear in the colour volume at each hit point, NaN without a colour).  Every live
pixel with a geometric pair adds lambda times its intensity residual against the bilinear interpolant of the
prediction's Y, so a flat textured wall, whose geometry leaves t_x, t_y and r_z free, is tracked.
`icp_max_intensity_difference` gates |r_I|; `prediction_colour` keeps the last colour image.  lambda has no default
other than off: no value is right across scenes.
With `icp_pyramid`, `icp_intensity_pyramid` (a rigid_opt.IntensityPyramid of the same levels) and `photometric_weight`
the joint solve runs on the depth pyramid (device_icp.icp_run_pyramid_photometric;
tests/pyramid_photometric_restatement.py restates it): the tracker builds an intensity pyramid of the frame's colour
image and one of the prediction's Y (2 x 2 means, NaN where one of the four has no colour), and a pixel of level L takes
its intensity term at level L of both with that level's intrinsics; `icp_max_normal_angle` still gates the geometric
pairs.  Without an `icp_intensity_pyramid` the combination is refused, since then there is no intensity pyramid to
take the term from.  Fusion still integrates the raw depth, `confidence` still shares the tracker's depth pyramid and
`prediction_colour` is kept.
With `icp_robust` (a rigid_opt.RobustLoss; tracking_reference="icp" only) the tracker's solve, in any of the
configurations above, is iteratively reweighted ("Robust ICP"; device_icp.icp_run_robust and
icp_run_pyramid_robust; tests/robust_icp_restatement.py restates it): every pair's rows are scaled by the Huber or
Tukey weight of its own residual at the current twist, so a part of the scene that moves against the rest -- whose
pairs sit inside the distance gate -- does not drag the pose the non-rigid step then has to undo.  The ICP records carry
weight_sum, photometric_weight_sum and outliers.  The scale has no default: none is right across sensors.  Fusion
itself is unchanged.
With a `nonrigid_optimizer` that is a HierarchicalOptimizer3d, every frame k >= 1 is fused through its warp field
("Warped depth fusion"; tests/warped_fusion_restatement.py restates it).  After tracking, the
live volume under the twist is generated (device_rigid.live_volume_3d), `psi = optimizer.optimize(model.tsdf, live)` is
the cumulative displacement in voxels with live(v + psi(v)) ~ model(v), a float32 (Z, Y, X, 3) device tensor (x, y, z
channels), and the frame is fused in depth mode with "the voxel's centre" replaced by "the voxel's warped point":
    point(v) = float32((float64(v) + float64(psi(v)) + array_offset) * voxel_size),   per axis
is transformed by the twist, projected, and the depth, the pixel weight and the colour are read at its pixel; the
weighted, carving and colour rules then apply unchanged (csrc/lsf_fusion.hip, lsf_fusion_integrate_depth_warped).  Nothing
is warped as a volume, so `carve`, `confidence` and `colour` combine with this optimizer (and with the one of the next
paragraph), and with no other.  A voxel
whose psi is not finite is left alone and counted in the record's warp_rejected (unpack_warped_record); psi = 0 gives
the unwarped calls bit for bit.  Frame 0 is fused as without an optimizer; `warp` keeps the last psi.
CanonicalVolume.integrate_depth(..., warp=) is the same call for a given field.  In 3-D the optimizer's default
tikhonov_strength = 0.2 diverges: its recursion g <- data - s * laplace(g) has gain 12 s at the highest frequency of the
7-point Laplacian, so s must lie below 1 / 12; 0.05 is stable.
With a SlavchevaOptimizer3d made with `cumulative_warp=True` (the KillingFusion iteration; INTEGRATION.md section 3,
"Cumulative warp"; tests/cumulative_warp_restatement.py restates it) frames k >= 1 are fused the same way: after tracking,
the live volume under the twist is generated, `optimizer.optimize(live, model.tsdf)` runs -- every iteration re-warps the
live volume by its own update u_k, and a composition launch behind it (csrc/lsf_cumulative_warp.hip) keeps
PSI_{k+1}(v) = u_k(v) + PSI_k(v + u_k(v)), PSI_0 = 0 --, `warp` takes `optimizer.cumulative_warp_field`, the total
displacement with live(v + PSI(v)) ~ model(v), and the frame is fused in depth mode through it, with `carve`, `confidence`
and `colour` as set.  The warped live volume itself is dropped.  On a model fused from depth the level-set term is best
left off (level_set_term_enabled=False): the voxels behind the model's band were never observed and keep the initial +1
where the live volume has -1, the term's gradient of the live field is huge across that step, and on
tests/deforming_scene.py it produces updates of 14 voxels per iteration, after which the chain changes the model by 0.17
per voxel near the surface, against 0.070 with the term off and 0.212 fused rigidly.  That is the reference's term doing
what it does on such a field, not a fault of the composition.  The keyword is refused together with
sobolev_smoothing_enabled and with a slab `comm`.
With any other non-rigid optimizer (a SlavchevaOptimizer3d without that keyword, in a KillingFusion or SobolevFusion
configuration: its final warp_field is the last iteration's update only, not a cumulative warp) the live volume under the
twist is generated,
warped into the model by `nonrigid_optimizer.optimize(live, model.tsdf)`, and fused in volume mode: unweighted,
uncarved, uncoloured -- `carve`, `confidence` and `colour` raise with it, since the observation mask, the weights and
the colour would have to be warped with the live field.

Moving volume ("Moving volume"; tests/volume_shift_restatement.py restates it): all of the above
happens in one box, fixed in the world by field_shape and array_offset.  SequenceFusion3d(..., moving_volume=
MovingVolume(threshold_voxels, anchor)) makes it a window that follows the camera in whole-voxel steps.  After a frame
is fused the policy takes `anchor`, a point in camera coordinates some way in front of the lens, to world coordinates
with the frame's twist; when it lies more than threshold_voxels from the window's centre on any axis, the window moves
by trunc of that distance on every axis.  CanonicalVolume.shift(s, array_offset) then copies the model shifted by s into
its spare buffers (one launch of csrc/lsf_volume_shift.hip: dst(v) = src(v + s), empty where v + s leaves the volume)
and swaps them in, and `array_offset` becomes array_offset + s (`initial_array_offset` keeps the first).  A voxel's
world point is float32((float64(v) + array_offset) * voxel_size), so a retained voxel keeps it bit for bit and every
later fusion is the one a fixed volume would have made there.  With the policy's stream_mesh the cells that leave are
meshed first -- at most three boxes, each through extract_mesh's kernels with their host read -- and appended to
`streamed_meshes` as host tuples; extract_mesh(include_streamed=True) is merge_meshes of the window's mesh and those
chunks.  Every cell is drawn exactly once; the vertices on a seam appear on both sides, and since the window goes on
fusing the layer a chunk was cut along, later frames can open hairline cracks there (Kintinuous has the same property).
The frame record gains "shift" and "streamed_faces", only with a moving_volume.  The shift sits between frames, so it
combines with every tracking mode and every non-rigid setting; `warp` and `prediction` remain the last frame's, in the
window that frame had.  Cost: profiles/moving_volume_cost.md.

Brick store ("Brick store"; tests/volume_bricks_restatement.py restates it): opt-in, the window
made lossless.  The world is cut into bricks of 8 voxels per axis on an integer lattice that a BrickStore fixes at its
first use (`origin`, the array_offset of the first shift that uses it; every later window must lie whole voxels from it).
CanonicalVolume.shift(..., brick_store=store) compacts the bricks that hold a voxel which leaves with data
(csrc/lsf_volume_bricks.hip: a count with one host read of the total, then a gather), copies them to the host and merges
them into the store, shifts as above, and writes the store's bricks that touch what entered back into the new buffers
(a scatter in place), clearing them in the store: a lattice voxel with data lives in exactly one place, the window or
the store.  A voxel holds data when its weight is non-zero (a NaN counts); one that leaves without data is not kept
and comes back as the empty voxel (tsdf 1, weight 0, colour 0).  CanonicalVolume.assemble(store, array_offset) builds
window plus store as fresh dense device tensors over their bounding box.  MovingVolume(..., stream_mesh=False,
keep_tsdf=True) makes SequenceFusion3d own `brick_store` and pass it to every shift -- the frame records gain bricks_out
and bricks_in -- and extract_mesh(include_streamed=True) then meshes the assembled map: one mesh without seams, at the
caller's iso, min_weight, normals and colours.  keep_tsdf does not combine with stream_mesh (a re-entered region would be
meshed twice).  Cost: profiles/volume_bricks_cost.md.

RGB-D sensor ("RGB-D sensor"; tests/rgbd_restatement.py restates it): everything above assumes
that one ideal pinhole camera made both images.  RgbdSensor(depth_camera, colour_camera, depth_to_colour) stands in front
of it for a real sensor -- two lenses with distortion, apart, of different resolutions.  sensor.register(depth_image,
colour_image) registers the raw depth into the RECTIFIED colour camera (csrc/lsf_rgbd.hip: every depth pixel lifted along
its undistorted ray, moved by q = R p + t, and its projected quad's bounding box splatted through an unsigned-minimum
z-buffer) and resamples the raw colour into the same ideal camera; a pixel without an answer has depth 0, which every
kernel here already reads as "no measurement".  SequenceFusion3d(None, ..., sensor=sensor) does that to every raw pair
given to integrate and then runs the frame unchanged on sensor.camera: every tracking mode, carve, confidence, the
pyramids, moving_volume and the non-rigid steps see the registered stream, and the frame record gains "registration", the
call's eight counts.  With colour=False the sensor gets no colour image; the depth is still registered into the colour
camera when the sensor has one.  Without the keyword nothing changes.  Cost: profiles/rgbd_sensor_cost.md.

Tracking quality and relocalisation ("Tracking quality and relocalisation";
tests/relocaliser_restatement.py restates it): without them every tracker result is trusted.  With
SequenceFusion3d(tracking_quality=TrackingQuality(min_pair_fraction, max_rms)), in "icp" and "sdf" mode, a frame k >= 1 is
judged by its last ICP record: good when the record is not skipped, count * s^2 / (H * W) >= min_pair_fraction (s the
stride of the record's level) and sqrt(energy / count) <= max_rms.  A frame that is not good is not fused and takes no
non-rigid step, its twist in `twists` is the last good twist, and the next frame starts from there; the frame record
gains tracking_state ("tracking" or "lost") and tracking_quality (pair_fraction, rms, skipped), and its fusion is None
when nothing was fused.  relocaliser=Relocaliser(...) (it implies TrackingQuality(); refused with a moving_volume, whose
window a keyframe's view may have left) adds the way back: every frame is encoded into a coarse image of block means
and, when fused, offered to a database of keyframes encoded by random ferns (csrc/lsf_relocaliser.hip: lsf_reloc_encode,
lsf_reloc_query), which keeps the frames that are far from all it holds, with their twists.  A frame that is not good,
or that follows a lost one, is tracked again from the nearest keyframes' twists in order and last from the last good
twist (not again, when it has just failed from it); the first good result makes it "relocalised", none leaves it
"lost".  From a relocalisation on, Relocaliser(resume_after=) good frames, the relocalised one included, are tracked
but not fused ("recovering").  The record gains keyframe and relocalisation.  Without the keywords nothing changes, and
no record has a new key.  Cost: profiles/relocaliser_cost.md.

Host synchronisations per frame: the rigid run's or the ICP run's one copy back (frames >= 1 with rigid_iterations > 0,
or with icp_iterations summing to > 0 in "icp" mode; in "raycast" and "icp" mode it also brings the prediction's hit
count), the non-rigid optimize()'s own (when one is given), and one read of
the fusion record.  CanonicalVolume.extract_mesh (and SequenceFusion3d.extract_mesh) costs one: the read of the
vertex and face totals.  A moving volume's policy adds none (the twist is on the host already); a shift that streams
costs extract_mesh's one per leaving box, at most three, and the chunks' copies to the host; a shift with a brick
store costs one, the read of the brick total, and the copies of the gathered rows to the host and of the re-entering
bricks to the card.  A sensor adds none per frame (its record is read with the fusion record's wait); its first frame
waits once for the check of the ray tables.  A tracking_quality adds none (the records are on the host); a relocaliser adds
one 48-byte copy per query: one per fused frame, one more per frame that has to be relocalised, and a tracker run per
start that is tried.

Not covered: carving, weights or colour in volume mode, a cumulative warp out of SobolevFusion
(sobolev_smoothing_enabled) or out of a z-slab / multi-GPU run (`comm`), a carve-distance
limit, keeping the warp field between frames as a warm start, ray-casting or meshing in the live frame, a whole frame
enqueued without host synchronisations, z-slab / multi-GPU fusion, a 2-D depth-mode row generator, fusing the filtered
depth, a downsampled prediction depth and normal pyramid (every level still pairs into the full-resolution
prediction), for the robust ICP weights a scale estimated from the residuals (MAD or the previous iteration's RMS),
the weight image used as `pixel_weight` in fusion and robust weights in the SDF-2-SDF trackers, smoothing the intensity
before level 0, ICP combined
with SDF-2-SDF, for the "sdf" tracker through the sequence's own `icp_*` and `photometric_weight` keywords a depth
pyramid or filtered depth as the point source and a colour term against the colour volume (both are settings of the
`sdf_tracker`), a normal-angle gate from the SDF gradient,
a minimum-weight gate and a per-voxel weight on the pairs, an adaptive ray-casting step, a confidence
image in the prediction, for the RGB-D sensor fisheye and thin-prism lens models, registering colour into the depth
camera, hole filling, time synchronisation of the two streams, rolling shutter and the reference's XML calibration
files, marching squares for 2-D models, vertex attributes beyond normals and
colours, welding vertices by position, decimation, a mesh extracted without the host read of its totals, for the
relocaliser relocalising inside a moving window, saving the keyframe database, loop closure and a learned quality
test, and for the moving volume welding across seams, a shift enqueued without the mesh totals' host read, and for its
brick store saving the store to disk, streaming without the host read of the brick total, and bricks in half
precision."""
import math

import numpy as np
import torch

from .. import (device_depth_confidence, device_fusion, device_icp, device_mesh, device_raycast, device_rigid,
                device_rgbd, device_volume_bricks, device_volume_shift)
from ..device_core import require_gpu
from ..device_fusion import (COLOUR_RECORD_FIELDS, RECORD_FIELDS, WARPED_RECORD_FIELDS, WEIGHTED_RECORD_FIELDS,
                             unpack_colour_record, unpack_record, unpack_warped_record, unpack_weighted_record)
from ..nonrigid_opt.hierarchical.hierarchical_optimizer3d import HierarchicalOptimizer3d
from ..nonrigid_opt.slavcheva.slavcheva_optimizer3d import SlavchevaOptimizer3d
from ..rigid_opt.depth_pyramid import DepthPyramid
from ..rigid_opt.frame_tracker import device_colour_image
from ..rigid_opt.point_to_sdf3d import PointToSdf3d
from ..rigid_opt.projective_icp3d import ProjectiveIcp3d
from ..rigid_opt.sdf_2_sdf_optimizer3d import unpack_record as unpack_rigid_record
from .._lib import DEPTH_F32
from ..math_utils.transformation import twist_vector_to_matrix3d
from ..tsdf.generation import DepthCamera, device_depth, offsets_of
from .brick_store import BrickStore
from .relocaliser import Relocaliser, TrackingQuality, level_stride
from .rgbd_sensor import RgbdSensor

__all__ = ["CanonicalVolume", "SequenceFusion3d", "DepthConfidence", "MovingVolume", "BrickStore", "RgbdSensor",
           "Relocaliser", "TrackingQuality",
           "merge_meshes",
           "unpack_record", "unpack_weighted_record",
           "unpack_colour_record", "unpack_warped_record", "RECORD_FIELDS", "WEIGHTED_RECORD_FIELDS",
           "COLOUR_RECORD_FIELDS", "WARPED_RECORD_FIELDS",
           "TRACKING_REFERENCES", "TRACKING_MODES", "DIRECT_TRACKING_MODES"]

# the trackers with a reference volume (rigid_run_3d), with them the one that tracks against a prediction image, and
# the ones that read the model directly; SequenceFusion3d accepts the union
TRACKING_REFERENCES = ("model", "raycast")
TRACKING_MODES = TRACKING_REFERENCES + ("icp",)
DIRECT_TRACKING_MODES = ("sdf",)


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


def _filter_settings(pyramid):
    """what decides a pyramid's level 0: the filter and the normals' gate"""
    return pyramid.radius, pyramid.sigma_space, pyramid.sigma_range, pyramid.depth_gate


class DepthConfidence:
    """the settings of the per-pixel confidence image c = |n . r| min(1, (reference_depth / z)^2)
    (device_depth_confidence.depth_confidence).  reference_depth: metres, finite and > 0, the depth up to which a
    frontal pixel counts fully; pyramid: a rigid_opt.DepthPyramid whose filter settings give the level-0 depth and
    normals (its levels are not used), DepthPyramid()'s own by default."""

    def __init__(self, reference_depth=device_depth_confidence.REFERENCE_DEPTH, pyramid=None):
        self.reference_depth = device_depth_confidence.checked_reference_depth(reference_depth)
        if pyramid is not None and not isinstance(pyramid, DepthPyramid):
            raise ValueError("pyramid must be a rigid_opt.DepthPyramid or None, got %r" % (pyramid,))
        self.pyramid = DepthPyramid() if pyramid is None else pyramid

    def shares(self, pyramid):
        """whether level 0 of `pyramid` (a DepthPyramid or None) is the one this confidence is computed from"""
        return pyramid is not None and _filter_settings(pyramid) == _filter_settings(self.pyramid)

    def from_levels(self, levels, camera):
        """the float32 (H, W) device weight image of a built pyramid's level 0 (a PyramidLevels), enqueued"""
        return device_depth_confidence.depth_confidence(levels.depth[0], levels.normals[0], camera,
                                                        self.reference_depth)

    def build_device(self, depth, code, camera):
        """the weight image of a device depth image and its LSF_DEPTH_* code: a one-level pyramid, then from_levels"""
        settings = dict(self.pyramid.settings(), levels=1)
        return self.from_levels(DepthPyramid(**settings).build_device(depth, code, camera), camera)

    def build(self, depth_image, camera):
        """build_device of a depth image (uint16 / float32 / float64, numpy or device)"""
        require_gpu()
        return self.build_device(*device_depth(depth_image), camera)


def _on_device(x, name, dtype, move=True):
    """x, a numpy array of `dtype` or a tensor, as a device tensor.  move=False leaves a tensor where it is: a CPU
    tensor is then refused by the device check of the call, not moved"""
    if isinstance(x, torch.Tensor):
        return x.to("cuda") if move and not x.is_cuda else x
    a = np.asarray(x)
    if a.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, np.dtype(dtype).name, a.dtype))
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


class MovingVolume:
    """the policy of a window that follows the camera in whole-voxel steps (module docstring, "Moving volume").  Host
    only.  threshold_voxels: positive; the window stays while the anchor is within that many voxels of its centre on
    every axis.  anchor: the point in CAMERA coordinates (metres) the window keeps near its centre, (0, 0, depth) some
    way in front of the lens -- the model is where the camera looks; it has no default, since no depth is right
    across scenes.  stream_mesh, min_weight, normals: whether and how SequenceFusion3d meshes the cells that leave.
    keep_tsdf: SequenceFusion3d keeps what leaves with data in it as bricks (its `brick_store`) and writes back what
    the window re-enters; it does not combine with stream_mesh, which would mesh a re-entered region twice, and since
    stream_mesh defaults to True, keep_tsdf=True needs stream_mesh=False said explicitly."""

    def __init__(self, threshold_voxels, anchor, stream_mesh=True, min_weight=0.0, normals=False, keep_tsdf=False):
        if keep_tsdf and stream_mesh:
            raise ValueError("keep_tsdf=True does not combine with stream_mesh=True (a region the window re-enters "
                             "would be meshed twice); stream_mesh defaults to True, so pass stream_mesh=False "
                             "explicitly with keep_tsdf=True")
        self.keep_tsdf = bool(keep_tsdf)
        self.threshold_voxels = float(threshold_voxels)
        if not (np.isfinite(self.threshold_voxels) and self.threshold_voxels > 0):
            raise ValueError("threshold_voxels must be finite and positive, got %r" % (threshold_voxels,))
        a = np.asarray(anchor, dtype=np.float64).reshape(-1)
        if a.size != 3 or not np.all(np.isfinite(a)):
            raise ValueError("anchor must be three finite camera coordinates in metres, got %r" % (anchor,))
        self.anchor = a.copy()
        self.min_weight = float(min_weight)
        if np.isnan(self.min_weight):
            raise ValueError("min_weight must not be NaN")
        self.stream_mesh, self.normals = bool(stream_mesh), bool(normals)

    def shift_for(self, twist, array_offset, shape, voxel_size):
        """(sx, sy, sz), Python ints, all zero for "stay".  The anchor goes to world coordinates by the inverse of
        twist_vector_to_matrix3d of the float32-rounded twist (the generator's convention, raycast's); d is its
        position in voxels minus the window's centre array_offset + (n - 1) / 2 per axis, in float64.  While no |d_j|
        exceeds the threshold the window stays; otherwise the shift is trunc(d_j) on EVERY axis, so one shift
        re-centres all three and shifts stay rare.  shape is the model's (Z, Y, X)."""
        if len(shape) != 3:
            raise ValueError("a moving volume needs a 3-D (Z, Y, X) model, got shape %s" % (tuple(shape),))
        if not (np.isfinite(voxel_size) and voxel_size > 0):
            raise ValueError("voxel_size must be finite and positive")
        t32 = np.asarray(twist, dtype=np.float64).reshape(6).astype(np.float32)
        m = twist_vector_to_matrix3d(t32)  # world -> camera
        rot, t = m[:3, :3].astype(np.float64), m[:3, 3].astype(np.float64)
        world = rot.T @ (self.anchor - t)
        n = np.array([shape[2], shape[1], shape[0]], dtype=np.float64)  # x, y, z
        d = world / float(voxel_size) - (offsets_of(array_offset) + (n - 1.0) / 2.0)
        if not np.all(np.isfinite(d)):
            raise ValueError("the anchor's world position is not finite under twist %r" % (twist,))
        if not np.any(np.abs(d) > self.threshold_voxels):
            return (0, 0, 0)
        return tuple(int(v) for v in np.trunc(d))


def _mesh_layout(mesh):
    """(with normals, with colours) of a host mesh tuple in extract_mesh's layout: (V, F), (V, F, N), (V, F, C) or
    (V, F, N, C), C being uint8"""
    if not isinstance(mesh, (tuple, list)) or not 2 <= len(mesh) <= 4:
        raise ValueError("a mesh is a tuple (vertices, faces[, normals][, colours])")
    extras = [np.asarray(a) for a in mesh[2:]]
    coloured = bool(extras) and extras[-1].dtype == np.uint8
    with_normals = len(extras) - int(coloured) == 1
    if len(extras) - int(coloured) not in (0, 1):
        raise ValueError("a mesh is a tuple (vertices, faces[, normals][, colours])")
    return with_normals, coloured


def merge_meshes(meshes):
    """the concatenation of host meshes in extract_mesh's layout (numpy tuples (vertices, faces[, normals][, colours])):
    vertices, normals and colours stacked in order, every mesh's face indices offset by the vertices before it.
    Nothing is welded.  Meshes of different layouts are refused, and so is an empty list: it has no layout."""
    meshes = list(meshes)
    if not meshes:
        raise ValueError("merge_meshes needs at least one mesh")
    layout = _mesh_layout(meshes[0])
    for m in meshes[1:]:
        if _mesh_layout(m) != layout:
            raise ValueError("merge_meshes needs meshes of one layout (normals and colours in all or in none)")
    counts = [len(m[0]) for m in meshes]
    if sum(counts) > 0x7fffffff:
        raise ValueError("the merged mesh has more vertices than int32 face indices reach")
    bases = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
    out = [np.concatenate([np.asarray(m[0], dtype=np.float32).reshape(-1, 3) for m in meshes]),
           np.concatenate([np.asarray(m[1], dtype=np.int32).reshape(-1, 3) + b for m, b in zip(meshes, bases)])]
    for j in range(2, len(meshes[0])):
        out.append(np.concatenate([np.asarray(m[j]).reshape(-1, 3) for m in meshes]))
    return tuple(out)


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
        depth_image's shape, numpy or device) and carve choose the weighted rule (module docstring), whose record
        unpack_weighted_record reads; with neither the call is the unweighted one.  colour_image (uint8 (H, W, 3),
        numpy or device, registered to depth_image; the volume must have been made with colour=True) also fuses colour
        inside (-colour_band, colour_band), the geometry as the weighted rule does; unpack_colour_record reads its
        record.  warp (float32, the model's shape + (3,), numpy or device: x, y, z displacement in voxels, what
        HierarchicalOptimizer3d.optimize(model, live) returns) makes every voxel observe the frame at its displaced
        point, by the weighted rule and with colour_image the colour rule (module docstring); unpack_warped_record
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
                     colours=False, default_colour=device_mesh.DEFAULT_COLOUR):
        """the level set iso of the model as a triangle mesh, with raycast's conventions (voxel (i, j, k) at
        ((k, j, i) + array_offset) * voxel_size): float32 vertices (V, 3) in world metres, (x, y, z); int32 faces
        (F, 3), their right-hand normal towards larger tsdf; with normals=True also the float32 unit normals (V, 3).
        Only cells whose 8 corners have weight > min_weight draw.  Returns (vertices, faces) or (vertices, faces,
        normals): device tensors with as_tensor=True, numpy copies otherwise.  With colours=True (a volume made with
        colour=True) the uint8 vertex colours (V, 3) are appended, row i the colour of vertex i, default_colour where
        neither end of the vertex's grid edge has a colour.  One host synchronisation: the read of the two totals."""
        if len(self.shape) != 3:
            raise ValueError("mesh extraction needs a 3-D model, this one has shape %s" % (self.shape,))
        if not colours:
            verts, faces, out_normals = device_mesh.extract_mesh(self.tsdf, self.weight, array_offset, voxel_size, iso,
                                                                 min_weight, normals)
            out = (verts, faces, out_normals) if normals else (verts, faces)
        else:
            if self.colour is None:
                raise ValueError("colours=True needs a volume made with colour=True")
            verts, faces, out_normals, out_colours = device_mesh.extract_mesh(
                self.tsdf, self.weight, array_offset, voxel_size, iso, min_weight, normals, self.colour, default_colour)
            out = (verts, faces, out_normals, out_colours) if normals else (verts, faces, out_colours)
        if not as_tensor:
            out = tuple(t.cpu().numpy() for t in out)
        return out

    def _leaving_mesh(self, box, array_offset, voxel_size, min_weight, normals, colours):
        """the host mesh of one box of leaving cells ((x0, x1), (y0, y1), (z0, z1)): extract_mesh of a contiguous copy
        of its voxels -- the cells' range plus one layer on the high side -- with array_offset moved by its origin"""
        (x0, x1), (y0, y1), (z0, z1) = box
        part = (slice(z0, z1 + 1), slice(y0, y1 + 1), slice(x0, x1 + 1))
        colour = self.colour[part].contiguous() if colours else None
        out = device_mesh.extract_mesh(self.tsdf[part].contiguous(), self.weight[part].contiguous(),
                                       offsets_of(array_offset) + np.array([x0, y0, z0], dtype=np.float64),
                                       voxel_size, 0.0, min_weight, normals, colour)
        keep = [out[0], out[1]] + ([out[2]] if normals else []) + ([out[3]] if colours else [])
        return tuple(t.cpu().numpy() for t in keep)

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


class SequenceFusion3d:
    """track each depth frame against the model (tracking_reference "model"), the live volume of its ray-cast
    prediction ("raycast"), by point-to-plane ICP the prediction's depth and normals ("icp") or, point to signed
    distance, the model's tsdf and weight ("sdf"), and fuse it (module docstring).  Keeps `canonical` (the
    CanonicalVolume), `twists` (one float64 (6,) per frame),
    `frame_records` (one dict per frame: frame, twist, rigid_records, nonrigid, fusion, prediction_hits -- the pixels
    of the prediction that hit the model, None without a prediction), in "raycast" and "icp" mode `prediction`
    (the last predicted depth image, a float32 device tensor in metres) and, with a HierarchicalOptimizer3d as the
    non-rigid step, or a SlavchevaOptimizer3d made with cumulative_warp=True, `warp` (the last frame's displacement
    field, a float32 (Z, Y, X, 3) device tensor; None before frame 1).  In "icp" mode rigid_records holds the ICP
    records (device_icp.unpack_record); with photometric_weight they carry photometric_count and photometric_energy,
    and `prediction_colour` is the last prediction's float32 (H, W, 4) colour image; with icp_intensity_pyramid the
    joint solve runs on the icp_pyramid (`icp.last_intensity_pyramids` keeps the two intensity pyramids); with
    icp_robust the solve is reweighted by that RobustLoss and the records carry weight_sum, photometric_weight_sum
    and outliers.  In "sdf" mode rigid_records holds `sdf_tracker`'s records, in the same layout.  With moving_volume
    (a MovingVolume) the model is a window that follows the camera: `array_offset` moves in whole voxels
    (`initial_array_offset` keeps the construction value), the frame records carry shift and streamed_faces, and
    `streamed_meshes` lists the host meshes of what left (module docstring, "Moving volume").  With sensor (an
    RgbdSensor) integrate takes the RAW frame pair, registers it first and runs the frame on the registered pair;
    `camera` may then be None and is sensor.camera, and the frame records carry registration (module docstring,
    "RGB-D sensor").  With tracking_quality (a TrackingQuality; "icp" and "sdf" mode) a frame whose last ICP record
    fails the gate is not fused and keeps the last good twist, `tracking_state` is the last frame's state and the
    records carry tracking_state and tracking_quality; with relocaliser (a Relocaliser) fused frames become keyframes
    and a lost frame is tracked again from the nearest keyframes' twists, the records carrying keyframe and
    relocalisation (module docstring, "Tracking quality and relocalisation")."""

    def __init__(self, camera, field_shape, array_offset, voxel_size=0.004, narrow_band_width_voxels=20,
                 max_weight=math.inf, rigid_iterations=60, rigid_rate=0.5, eta=0.01, nonrigid_optimizer=None,
                 initial_twist=None, tracking_reference="model", icp_iterations=device_icp.ITERATIONS,
                 icp_strides=device_icp.STRIDES, icp_max_distance=device_icp.MAX_DISTANCE, icp_pyramid=None,
                 icp_max_normal_angle=None, carve=False, confidence=None, colour=False, colour_band=1.0,
                 photometric_weight=None, icp_max_intensity_difference=math.inf, icp_intensity_pyramid=None,
                 icp_robust=None, sdf_tracker=None, moving_volume=None, sensor=None, tracking_quality=None,
                 relocaliser=None):
        if sensor is not None:
            if not isinstance(sensor, RgbdSensor):
                raise ValueError("sensor must be a fusion.RgbdSensor or None, got %r" % (sensor,))
            if camera is not None and camera is not sensor.camera:
                raise ValueError("a sequence with a sensor runs on sensor.camera, the camera of the registered stream: "
                                 "pass camera=None (or sensor.camera)")
            camera = sensor.camera
        elif camera is None:
            raise ValueError("camera may be None only with a sensor")
        self.sensor = sensor
        if moving_volume is not None and not isinstance(moving_volume, MovingVolume):
            raise ValueError("moving_volume must be a fusion.MovingVolume or None, got %r" % (moving_volume,))
        self.moving_volume = moving_volume
        if confidence is not None and not isinstance(confidence, DepthConfidence):
            raise ValueError("confidence must be a fusion.DepthConfidence or None, got %r" % (confidence,))
        self.carve, self.confidence = bool(carve), confidence
        # the optimizers that give a cumulative warp: their frames are fused through it, in depth mode
        self._composed = isinstance(nonrigid_optimizer, SlavchevaOptimizer3d) and nonrigid_optimizer.cumulative_warp
        self.warped = isinstance(nonrigid_optimizer, HierarchicalOptimizer3d) or self._composed
        volume_mode = nonrigid_optimizer is not None and not self.warped
        if volume_mode and (self.carve or confidence is not None):
            raise ValueError("carve and confidence need depth-mode fusion and do not combine with a nonrigid_optimizer: "
                             "volume-mode carving needs an observation mask warped with the live field")
        self.colour = bool(colour)
        if volume_mode and self.colour:
            raise ValueError("colour needs depth-mode fusion and does not combine with a nonrigid_optimizer: "
                             "the colour would have to be warped with the live field")
        self.colour_band = device_fusion.colour_band_of(colour_band)
        self.camera = camera
        self.field_shape = device_rigid.volume_shape(field_shape)
        self.array_offset = np.asarray(array_offset, dtype=np.float64).reshape(-1)
        if self.array_offset.size != 3:
            raise ValueError("array_offset must have 3 entries, got %d" % self.array_offset.size)
        self.initial_array_offset = self.array_offset.copy()  # a moving_volume moves array_offset; this one stays
        self.streamed_meshes = []  # a moving_volume with stream_mesh: the host meshes of the cells that left
        # a moving_volume with keep_tsdf: the bricks that left, written back when the window re-enters them
        self.brick_store = BrickStore(colour=bool(colour)) if moving_volume is not None and moving_volume.keep_tsdf \
            else None
        if not voxel_size > 0 or not narrow_band_width_voxels > 0:
            raise ValueError("voxel_size and narrow_band_width_voxels must be positive")
        if int(rigid_iterations) < 0:
            raise ValueError("rigid_iterations must be >= 0")
        modes = TRACKING_MODES + DIRECT_TRACKING_MODES
        if tracking_reference not in modes:
            raise ValueError("tracking_reference must be one of %s, got %r" % (modes, tracking_reference))
        if tracking_reference in DIRECT_TRACKING_MODES:
            for name, value in (("photometric_weight", photometric_weight), ("icp_robust", icp_robust),
                                ("icp_pyramid", icp_pyramid), ("icp_max_normal_angle", icp_max_normal_angle),
                                ("icp_intensity_pyramid", icp_intensity_pyramid)):
                if value is not None:
                    raise ValueError("%s belongs to the \"icp\" tracker, which pairs into a prediction image; "
                                     "tracking_reference=%r reads the model itself (a loss goes on the sdf_tracker: "
                                     "PointToSdf3d(robust=))" % (name, tracking_reference))
            if sdf_tracker is not None and not isinstance(sdf_tracker, PointToSdf3d):
                raise ValueError("sdf_tracker must be a rigid_opt.PointToSdf3d or None, got %r" % (sdf_tracker,))
        elif sdf_tracker is not None:
            raise ValueError("sdf_tracker needs tracking_reference=\"sdf\"")
        if photometric_weight is not None:
            if not self.colour or tracking_reference != "icp":
                raise ValueError("photometric_weight needs colour=True and tracking_reference=\"icp\"")
            if icp_pyramid is not None and icp_intensity_pyramid is None:
                raise ValueError("photometric_weight does not combine with an icp_pyramid: there is no intensity "
                                 "pyramid")
        if icp_robust is not None and tracking_reference != "icp":
            raise ValueError("icp_robust needs tracking_reference=\"icp\": the SDF-2-SDF trackers have no robust "
                             "weights")
        # the "icp" tracker; its arguments are checked in every mode
        t = self.icp = ProjectiveIcp3d(camera, icp_iterations, icp_strides, icp_max_distance, icp_pyramid,
                                       icp_max_normal_angle, photometric_weight, icp_max_intensity_difference,
                                       icp_intensity_pyramid, icp_robust)
        self.photometric_weight, self.icp_max_intensity_difference = t.photometric_weight, t.max_intensity_difference
        self.icp_iterations, self.icp_strides, self.icp_max_distance = t.iterations, t.strides, t.max_distance
        self.icp_pyramid, self.icp_max_normal_angle = t.pyramid, t.max_normal_angle
        self.icp_intensity_pyramid, self.icp_robust = t.intensity_pyramid, t.robust
        self.sdf_tracker = None
        if tracking_reference in DIRECT_TRACKING_MODES:
            self.sdf_tracker = PointToSdf3d(camera) if sdf_tracker is None else sdf_tracker
            if self.sdf_tracker.photometric_weight is not None and not self.colour:
                raise ValueError("an sdf_tracker with a photometric_weight needs colour=True: its colour term reads "
                                 "the model's colour volume")
        if tracking_quality is not None and not isinstance(tracking_quality, TrackingQuality):
            raise ValueError("tracking_quality must be a fusion.TrackingQuality or None, got %r" % (tracking_quality,))
        if relocaliser is not None:
            if not isinstance(relocaliser, Relocaliser):
                raise ValueError("relocaliser must be a fusion.Relocaliser or None, got %r" % (relocaliser,))
            if moving_volume is not None:
                raise ValueError("a relocaliser does not combine with a moving_volume: a keyframe's view may have left "
                                 "the window, and relocalising inside a moving window is out of scope")
            if tracking_quality is None:
                tracking_quality = TrackingQuality()
        if tracking_quality is not None and tracking_reference not in ("icp", "sdf"):
            raise ValueError("tracking_quality and relocaliser judge the ICP records of tracking_reference \"icp\" and "
                             "\"sdf\"; %r writes none" % (tracking_reference,))
        self.tracking_quality, self.relocaliser = tracking_quality, relocaliser
        self.tracking_state = "tracking"  # with a tracking_quality: the last frame's state
        self._recovering = 0  # with a relocaliser: the good frames still to pass unfused after a relocalisation
        self.voxel_size = voxel_size
        self.narrow_band_width_voxels = narrow_band_width_voxels
        self.rigid_iterations = int(rigid_iterations)
        self.rigid_rate = rigid_rate
        self.eta = eta
        self.nonrigid_optimizer = nonrigid_optimizer
        self.initial_twist = np.zeros(6) if initial_twist is None else device_rigid.twist6(initial_twist).copy()
        self.tracking_reference = tracking_reference
        self.canonical = CanonicalVolume(self.field_shape, max_weight, colour=self.colour)
        self.twists = []
        self.frame_records = []
        self.prediction = None  # "raycast", "icp": the last prediction, a float32 device depth image in metres
        self.prediction_colour = None  # photometric_weight: the last prediction's float32 (H, W, 4) colour image
        self.warp = None  # a warped step: the last frame's psi, a float32 (Z, Y, X, 3) device tensor
        self._previous = None  # "raycast": the previous frame's (device depth, LSF_DEPTH_* code)
        P = camera.intrinsics.intrinsic_matrix
        # the prediction is in metres: its live volume is generated with ratio 1
        self._metric_camera = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=P), depth_unit_ratio=1.0)

    def _prediction_volume(self, twist):
        """the live volume under twist of the model ray-cast at twist, holes filled from the previous frame; and the
        prediction's device hit count"""
        previous, code = self._previous
        model = self.canonical
        self.prediction, _, hits = device_raycast.raycast(model.tsdf, model.weight, self.camera, twist,
                                                          self.array_offset, self.voxel_size, tuple(previous.shape),
                                                          fallback_depth=previous, fallback_code=code)
        live = device_rigid.live_volume_3d(self.prediction, DEPTH_F32, self._metric_camera, self.field_shape,
                                           self.array_offset, twist, self.voxel_size, self.narrow_band_width_voxels)
        return live, hits

    def _track_icp(self, depth, code, twist, colour_image=None):
        """ICP of the frame against the model ray-cast with normals at twist (no fallback), started from twist: the
        new twist, the unpacked ICP records and the prediction's device hit count.  With photometric_weight the
        prediction carries the model's colour and the solve is the joint one, on the frame's colour_image"""
        model = self.canonical
        joint = self.photometric_weight is not None
        cast = device_raycast.raycast(model.tsdf, model.weight, self.camera, twist, self.array_offset, self.voxel_size,
                                      tuple(depth.shape), normals=True, colour=model.colour if joint else None)
        self.prediction, normals, hits = cast[:3]
        colours = {}
        if joint:
            self.prediction_colour = cast[3]
            colours = dict(colour_image=colour_image, prediction_colour=self.prediction_colour)
        twist, records, _ = self.icp.track(depth, code, self.prediction, normals, twist, twist, **colours)
        return twist, records, hits

    def _track_direct(self, depth, code, twist, colour_image, gen):
        """"icp" and "sdf" mode: the frame tracked from twist (the "icp" prediction is ray-cast at twist).  Returns the
        new twist, the unpacked records, the prediction's device hit count (None in "sdf" mode) and whether a tracker
        ran at all"""
        model = self.canonical
        if self.tracking_reference == "icp":
            if sum(self.icp_iterations) > 0:
                return self._track_icp(depth, code, twist,
                                       None if self.photometric_weight is None else colour_image) + (True,)
        elif sum(self.sdf_tracker.iterations) > 0:
            joint = {}
            if self.sdf_tracker.photometric_weight is not None:
                joint = dict(colour=model.colour, colour_image=colour_image)
            new, records, _ = self.sdf_tracker.track(depth, code, model.tsdf, model.weight, self.array_offset, twist,
                                                     **gen, **joint)
            return new, records, None, True
        return twist, [], None, False

    def _track_judged(self, depth, code, last_good, colour_image, gen, coarse, verdict):
        """a frame k >= 1 under a tracking_quality (module docstring, "Tracking quality and relocalisation"): tracked from
        the last good twist unless the state is lost, judged, and with a relocaliser tried again from the nearest
        keyframes' twists and last from the last good twist.  Returns _track_direct's tuple of the attempt that was
        good -- of the last attempt, with the last good twist, when none was -- and whether the frame is fused; fills
        verdict with state, quality and relocalisation"""
        tracker = self.icp if self.tracking_reference == "icp" else self.sdf_tracker
        shape = tuple(depth.shape)

        def attempt(start):
            out = self._track_direct(depth, code, start.copy(), colour_image, gen)
            last = out[1][-1] if out[1] else None
            stride = 1 if last is None else level_stride(tracker, last["level"])
            return out, self.tracking_quality.judge(last, shape, stride)

        reloc = self.relocaliser
        was_lost = reloc is not None and self.tracking_state == "lost"
        out, quality, state = None, None, "lost"
        if not was_lost:
            out, quality = attempt(last_good)
            if quality["good"]:
                state = "tracking"
        if state == "lost" and reloc is not None:
            found = reloc.query(coarse)
            verdict["relocalisation"] = {"candidates": found["nearest"], "distances": found["distances"],
                                         "chosen": None}
            starts = [(i, reloc.twists[i]) for i in found["nearest"]] + ([(-1, last_good)] if was_lost else [])
            for chosen, start in starts:  # the last good twist last; a frame that just failed from it is not tried again
                out, quality = attempt(start)
                if quality["good"]:
                    state = "relocalised"
                    verdict["relocalisation"]["chosen"] = chosen
                    self._recovering = reloc.resume_after
                    break
        good = state != "lost"
        fuse = good
        if good and self._recovering > 0:  # tracked, not fused: the model waits until the track has settled
            self._recovering -= 1
            fuse = False
            state = state if state == "relocalised" else "recovering"
        verdict["state"], verdict["quality"] = state, {k: quality[k] for k in ("pair_fraction", "rms", "skipped")}
        if not good:
            return last_good, out[1], out[2], out[3], False
        return out + (fuse,)

    def _frame_weight(self, depth, code, tracked):
        """the frame's confidence image (None without `confidence`): from the tracker's pyramid of this frame when it
        built one (tracked) with the confidence's filter settings, else from a one-level pyramid of its own"""
        c = self.confidence
        if c is None:
            return None
        if tracked and self.tracking_reference == "icp" and c.shares(self.icp_pyramid):
            return c.from_levels(self.icp.last_pyramid, self.camera)
        if tracked and self.tracking_reference == "sdf" and c.shares(self.sdf_tracker.pyramid):
            return c.from_levels(self.sdf_tracker.last_pyramid, self.camera)
        return c.build_device(depth, code, self.camera)

    def integrate(self, depth_image, colour_image=None):
        """track and fuse one frame; returns its record (also appended to frame_records).  A sequence made with
        colour=True needs the frame's colour_image (uint8 (H, W, 3), numpy or device), any other takes none"""
        if self.colour and colour_image is None:
            raise ValueError("a sequence made with colour=True needs a colour_image on every frame")
        if not self.colour and colour_image is not None:
            raise ValueError("colour_image needs a sequence made with colour=True")
        k = len(self.twists)
        registration = None
        if self.sensor is not None:  # the raw pair becomes the registered pair; everything below sees that stream
            depth_image, colour_image, registration = self.sensor.register_device(depth_image, colour_image)
        depth, code = device_depth(depth_image)
        sdf_joint = self.sdf_tracker is not None and self.sdf_tracker.photometric_weight is not None
        if self.photometric_weight is not None or sdf_joint:
            colour_image = device_colour_image(colour_image)  # once: the tracker and the fusion both read it
        model = self.canonical
        rigid_records, nonrigid, hits, tracked = [], None, None, False
        gen = dict(voxel_size=self.voxel_size, narrow_band_width_voxels=self.narrow_band_width_voxels)
        # with a tracking_quality: whether the frame is fused, and what the frame record gains
        fuse, verdict, coarse = True, {}, None
        if self.relocaliser is not None:
            coarse = self.relocaliser.encode(depth, self.camera, colour_image if self.colour else None)
        if k == 0:
            twist = self.initial_twist.copy()
        else:
            twist = self.twists[-1].copy()
            if self.tracking_quality is not None:
                twist, rigid_records, hits, tracked, fuse = self._track_judged(depth, code, twist, colour_image, gen,
                                                                               coarse, verdict)
            elif self.tracking_reference in ("icp", "sdf"):
                twist, rigid_records, hits, tracked = self._track_direct(depth, code, twist, colour_image, gen)
            elif self.rigid_iterations > 0:
                reference = model.tsdf
                if self.tracking_reference == "raycast":
                    reference, hits = self._prediction_volume(twist)
                twist, records = device_rigid.rigid_run_3d(
                    reference, depth, code, self.camera, self.array_offset, self.rigid_iterations, self.rigid_rate,
                    self.eta, self.voxel_size, self.voxel_size, self.narrow_band_width_voxels, twist=twist)
                rigid_records = [unpack_rigid_record(r) for r in records]
                del reference
        through = self.nonrigid_optimizer is not None and k > 0 and fuse  # the frame takes the non-rigid step
        if through:
            live = device_rigid.live_volume_3d(depth, code, self.camera, self.field_shape, self.array_offset, twist,
                                               **gen)
            if self._composed:  # the live volume is warped in place and dropped: the frame is fused through PSI
                self.nonrigid_optimizer.optimize(live, model.tsdf)
                self.warp = self.nonrigid_optimizer.cumulative_warp_field
                del live
            elif self.warped:
                self.warp = self.nonrigid_optimizer.optimize(model.tsdf, live)
                del live
            else:
                self.nonrigid_optimizer.optimize(live, model.tsdf)
            nonrigid = self.nonrigid_optimizer.engine.last_call
        if not fuse:  # a frame that is not good leaves the model alone
            record, unpack = None, None
        elif through and not self.warped:  # the live volume, warped into the model, is fused in volume mode
            record, unpack = device_fusion.integrate_volume(model.tsdf, model.weight, live, 1.0,
                                                            model.max_weight), unpack_record
        else:  # depth mode, through the frame's warp field when it has one
            record, unpack = device_fusion.integrate_depth_by_arguments(
                model.tsdf, model.weight, depth, code, self.camera, self.array_offset, twist, w=1.0,
                max_weight=model.max_weight, pixel_weight=self._frame_weight(depth, code, tracked), carve=self.carve,
                colour=model.colour, colour_image=device_colour_image(colour_image) if self.colour else None,
                colour_band=self.colour_band, warp=self.warp if through else None, **gen)
        frame = {"frame": k, "twist": np.asarray(twist, dtype=np.float64).reshape(6).copy(),
                 "rigid_records": rigid_records, "nonrigid": nonrigid,
                 "fusion": None if record is None else unpack(record.cpu().numpy()),
                 "prediction_hits": None if hits is None else int(hits.item())}
        if self.tracking_quality is not None:
            frame["tracking_state"] = self.tracking_state = verdict.get("state", "tracking")
            frame["tracking_quality"] = verdict.get("quality")
        if self.relocaliser is not None:
            frame["relocalisation"] = verdict.get("relocalisation")
            frame["keyframe"] = None
            if fuse:  # every fused frame may become a keyframe
                frame["keyframe"] = self.relocaliser.query(coarse, harvest=True, twist=frame["twist"])["appended"]
        if registration is not None:
            frame["registration"] = device_rgbd.unpack_record(registration.cpu().numpy())
        if self.moving_volume is not None:  # between frames: the policy reads the frame's twist, already on the host
            mv = self.moving_volume
            s = mv.shift_for(frame["twist"], self.array_offset, self.field_shape, self.voxel_size)
            self.array_offset, chunks = model.shift(s, self.array_offset, self.voxel_size, mv.stream_mesh,
                                                    mv.min_weight, mv.normals, colours=mv.stream_mesh and self.colour,
                                                    brick_store=self.brick_store)
            self.streamed_meshes.extend(chunks)
            frame["shift"] = s
            frame["streamed_faces"] = int(sum(len(c[1]) for c in chunks))
            if self.brick_store is not None:
                frame["bricks_out"] = self.brick_store.last["bricks_out"]
                frame["bricks_in"] = self.brick_store.last["bricks_in"]
        if self.tracking_reference == "raycast":
            self._previous = (depth, code)
        self.twists.append(frame["twist"].copy())
        self.frame_records.append(frame)
        return frame

    def extract_mesh(self, iso=0.0, min_weight=0.0, normals=False, as_tensor=False, colours=False,
                     default_colour=device_mesh.DEFAULT_COLOUR, include_streamed=False):
        """CanonicalVolume.extract_mesh of the model with the sequence's array_offset and voxel_size.  With
        include_streamed (a sequence made with a moving_volume that streams) the window's mesh is followed by the
        streamed chunks, merge_meshes of them all: host arrays only, and only as the chunks were made -- iso 0, the
        policy's min_weight and normals, colours exactly when the sequence has colour, the default default_colour;
        anything else raises, since the chunks cannot be drawn again.  With a moving_volume that has keep_tsdf,
        include_streamed meshes CanonicalVolume.assemble of the window and the brick store instead: one mesh of the
        whole map without seams, at the caller's iso, min_weight, normals and colours, as tensors too"""
        if not include_streamed:
            return self.canonical.extract_mesh(self.array_offset, self.voxel_size, iso, min_weight, normals, as_tensor,
                                               colours, default_colour)
        mv = self.moving_volume
        if mv is not None and mv.keep_tsdf:
            if colours and not self.colour:
                raise ValueError("colours=True needs a sequence made with colour=True")
            tsdf, weight, colour, offset = self.canonical.assemble(self.brick_store, self.array_offset)
            out = device_mesh.extract_mesh(tsdf, weight, offset, self.voxel_size, iso, min_weight, normals,
                                           *((colour, default_colour) if colours else ()))
            out = tuple(t for t, kept in zip(out, (True, True, normals, colours)) if kept)
            return out if as_tensor else tuple(t.cpu().numpy() for t in out)
        if mv is None or not mv.stream_mesh:
            raise ValueError("include_streamed needs a sequence made with a moving_volume that has stream_mesh=True")
        same = (not as_tensor and iso == 0.0 and float(min_weight) == mv.min_weight and bool(normals) == mv.normals
                and bool(colours) == self.colour
                and device_mesh.default_colour_of(default_colour) == device_mesh.DEFAULT_COLOUR)
        if not same:
            raise ValueError("include_streamed gives host meshes with the attributes the chunks were streamed with: "
                             "iso=0, min_weight=%r, normals=%r, colours=%r, the default default_colour, as_tensor=False"
                             % (mv.min_weight, mv.normals, self.colour))
        window = self.canonical.extract_mesh(self.array_offset, self.voxel_size, 0.0, mv.min_weight, mv.normals, False,
                                             self.colour)
        return merge_meshes([window] + self.streamed_meshes)
