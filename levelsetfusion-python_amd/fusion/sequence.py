"""SequenceFusion3d: a frame's stages -- register, track, the non-rigid step, fuse, judge, shift the window -- over a
CanonicalVolume (the package's docstring has the rules of each)."""
import collections
import math

import numpy as np

from .. import device_fusion, device_icp, device_mesh, device_raycast, device_rgbd, device_rigid
from ..device_fusion import unpack_record
from ..nonrigid_opt.hierarchical.hierarchical_optimizer3d import HierarchicalOptimizer3d
from ..nonrigid_opt.slavcheva.slavcheva_optimizer3d import SlavchevaOptimizer3d
from ..rigid_opt.frame_tracker import device_colour_image
from ..rigid_opt.point_to_sdf3d import PointToSdf3d
from ..rigid_opt.projective_icp3d import ProjectiveIcp3d
from ..rigid_opt.sdf_2_sdf_optimizer3d import unpack_record as unpack_rigid_record
from .._lib import DEPTH_F32
from ..tsdf.generation import DepthCamera, device_depth
from .brick_store import BrickStore
from .canonical_volume import CanonicalVolume, components_filtered, mesh_outputs, simplified, smoothed
from .depth_confidence import DepthConfidence
from .mesh_components import filter_mesh_components
from .mesh_simplify import simplify_mesh
from .mesh_smooth import smooth_mesh
from .moving_volume import MovingVolume, merge_meshes
from .relocaliser import Relocaliser, TrackingQuality, level_stride
from .rgbd_sensor import RgbdSensor

# the trackers with a reference volume (rigid_run_3d), with them the one that tracks against a prediction image, and
# the ones that read the model directly; SequenceFusion3d accepts the union
TRACKING_REFERENCES = ("model", "raycast")
TRACKING_MODES = TRACKING_REFERENCES + ("icp",)
DIRECT_TRACKING_MODES = ("sdf",)

# a frame's tracking step: the twist, the unpacked records, the prediction's device hit count (None without a
# prediction) and whether a tracker ran at all
Tracked = collections.namedtuple("Tracked", "twist records hits ran")


class SequenceFusion3d:
    """track each depth frame against the model (tracking_reference "model"), the live volume of its ray-cast
    prediction ("raycast"), by point-to-plane ICP the prediction's depth and normals ("icp") or, point to signed
    distance, the model's tsdf and weight ("sdf"), and fuse it (package docstring).  Keeps `canonical` (the
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
    `streamed_meshes` lists the host meshes of what left (package docstring, "Moving volume").  With sensor (an
    RgbdSensor) integrate takes the RAW frame pair, registers it first and runs the frame on the registered pair;
    `camera` may then be None and is sensor.camera, and the frame records carry registration (package docstring,
    "RGB-D sensor").  With tracking_quality (a TrackingQuality; "icp" and "sdf" mode) a frame whose last ICP record
    fails the gate is not fused and keeps the last good twist, `tracking_state` is the last frame's state and the
    records carry tracking_state and tracking_quality; with relocaliser (a Relocaliser) fused frames become keyframes
    and a lost frame is tracked again from the nearest keyframes' twists, the records carrying keyframe and
    relocalisation (package docstring, "Tracking quality and relocalisation")."""

    def __init__(self, camera, field_shape, array_offset, voxel_size=0.004, narrow_band_width_voxels=20,
                 max_weight=math.inf, rigid_iterations=60, rigid_rate=0.5, eta=0.01, nonrigid_optimizer=None,
                 initial_twist=None, tracking_reference="model", icp_iterations=device_icp.ITERATIONS,
                 icp_strides=device_icp.STRIDES, icp_max_distance=device_icp.MAX_DISTANCE, icp_pyramid=None,
                 icp_max_normal_angle=None, carve=False, confidence=None, colour=False, colour_band=1.0,
                 photometric_weight=None, icp_max_intensity_difference=math.inf, icp_intensity_pyramid=None,
                 icp_robust=None, sdf_tracker=None, moving_volume=None, sensor=None, tracking_quality=None,
                 relocaliser=None):
        if sensor is not None:  # the refusals first, none needs a GPU; what they convert on the way stays in a local
            if not isinstance(sensor, RgbdSensor):
                raise ValueError("sensor must be a fusion.RgbdSensor or None, got %r" % (sensor,))
            if camera is not None and camera is not sensor.camera:
                raise ValueError("a sequence with a sensor runs on sensor.camera, the camera of the registered stream: "
                                 "pass camera=None (or sensor.camera)")
            camera = sensor.camera
        elif camera is None:
            raise ValueError("camera may be None only with a sensor")
        if moving_volume is not None and not isinstance(moving_volume, MovingVolume):
            raise ValueError("moving_volume must be a fusion.MovingVolume or None, got %r" % (moving_volume,))
        if confidence is not None and not isinstance(confidence, DepthConfidence):
            raise ValueError("confidence must be a fusion.DepthConfidence or None, got %r" % (confidence,))
        # the optimizers that give a cumulative warp: their frames are fused through it, in depth mode
        composed = isinstance(nonrigid_optimizer, SlavchevaOptimizer3d) and nonrigid_optimizer.cumulative_warp
        warped = isinstance(nonrigid_optimizer, HierarchicalOptimizer3d) or composed
        volume_mode = nonrigid_optimizer is not None and not warped
        if volume_mode and (carve or confidence is not None):
            raise ValueError("carve and confidence need depth-mode fusion and do not combine with a nonrigid_optimizer: "
                             "volume-mode carving needs an observation mask warped with the live field")
        if volume_mode and colour:
            raise ValueError("colour needs depth-mode fusion and does not combine with a nonrigid_optimizer: "
                             "the colour would have to be warped with the live field")
        colour_band = device_fusion.colour_band_of(colour_band)
        field_shape = device_rigid.volume_shape(field_shape)
        array_offset = np.asarray(array_offset, dtype=np.float64).reshape(-1)
        if array_offset.size != 3:
            raise ValueError("array_offset must have 3 entries, got %d" % array_offset.size)
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
            if not colour or tracking_reference != "icp":
                raise ValueError("photometric_weight needs colour=True and tracking_reference=\"icp\"")
            if icp_pyramid is not None and icp_intensity_pyramid is None:
                raise ValueError("photometric_weight does not combine with an icp_pyramid: there is no intensity "
                                 "pyramid")
        if icp_robust is not None and tracking_reference != "icp":
            raise ValueError("icp_robust needs tracking_reference=\"icp\": the SDF-2-SDF trackers have no robust "
                             "weights")
        # the "icp" tracker; its arguments are checked in every mode
        icp = ProjectiveIcp3d(camera, icp_iterations, icp_strides, icp_max_distance, icp_pyramid,
                              icp_max_normal_angle, photometric_weight, icp_max_intensity_difference,
                              icp_intensity_pyramid, icp_robust)
        if tracking_reference in DIRECT_TRACKING_MODES:
            sdf_tracker = PointToSdf3d(camera) if sdf_tracker is None else sdf_tracker
            if sdf_tracker.photometric_weight is not None and not colour:
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
        initial_twist = np.zeros(6) if initial_twist is None else device_rigid.twist6(initial_twist).copy()

        self.sensor, self.camera, self.moving_volume = sensor, camera, moving_volume
        self.carve, self.confidence = bool(carve), confidence
        self._composed, self.warped = composed, warped
        self.colour, self.colour_band = bool(colour), colour_band
        self.field_shape, self.array_offset = field_shape, array_offset
        self.initial_array_offset = self.array_offset.copy()  # a moving_volume moves array_offset; this one stays
        self.streamed_meshes = []  # a moving_volume with stream_mesh: the host meshes of the cells that left
        self.mesh_records = dict(weld=None, simplify=None)  # extract_mesh(weld=, simplify_cell=): the last call's
        self.last_esdf_record = self.last_esdf_offset = None  # esdf: the last call's record and its field's array offset
        # a moving_volume with keep_tsdf: the bricks that left, written back when the window re-enters them
        self.brick_store = BrickStore(colour=bool(colour)) if moving_volume is not None and moving_volume.keep_tsdf \
            else None
        t = self.icp = icp
        self.photometric_weight, self.icp_max_intensity_difference = t.photometric_weight, t.max_intensity_difference
        self.icp_iterations, self.icp_strides, self.icp_max_distance = t.iterations, t.strides, t.max_distance
        self.icp_pyramid, self.icp_max_normal_angle = t.pyramid, t.max_normal_angle
        self.icp_intensity_pyramid, self.icp_robust = t.intensity_pyramid, t.robust
        self.sdf_tracker = sdf_tracker
        self.tracking_quality, self.relocaliser = tracking_quality, relocaliser
        self.tracking_state = "tracking"  # with a tracking_quality: the last frame's state
        self._recovering = 0  # with a relocaliser: the good frames still to pass unfused after a relocalisation
        self.voxel_size, self.narrow_band_width_voxels = voxel_size, narrow_band_width_voxels
        self._gen = dict(voxel_size=voxel_size, narrow_band_width_voxels=narrow_band_width_voxels)
        self.rigid_iterations, self.rigid_rate, self.eta = int(rigid_iterations), rigid_rate, eta
        self.nonrigid_optimizer, self.initial_twist = nonrigid_optimizer, initial_twist
        self.tracking_reference = tracking_reference
        self.canonical = CanonicalVolume(self.field_shape, max_weight, colour=self.colour)
        self.twists, self.frame_records = [], []
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

    def _track(self, depth, code, twist, colour_image):
        """the frame tracked from twist by the sequence's tracking_reference, a Tracked: "model" against the model's
        tsdf, "raycast" against the live volume of the prediction at twist, "icp" against the prediction ray-cast at
        twist, "sdf" against the model itself.  A tracker without iterations keeps the twist and writes no records"""
        mode, model = self.tracking_reference, self.canonical
        if mode == "icp":
            if sum(self.icp_iterations) > 0:
                joint = None if self.photometric_weight is None else colour_image
                return Tracked(*self._track_icp(depth, code, twist, joint), ran=True)
        elif mode == "sdf":
            if sum(self.sdf_tracker.iterations) > 0:
                joint = {}
                if self.sdf_tracker.photometric_weight is not None:
                    joint = dict(colour=model.colour, colour_image=colour_image)
                new, records, _ = self.sdf_tracker.track(depth, code, model.tsdf, model.weight, self.array_offset,
                                                         twist, **self._gen, **joint)
                return Tracked(new, records, None, True)
        elif self.rigid_iterations > 0:
            reference, hits = model.tsdf, None
            if mode == "raycast":
                reference, hits = self._prediction_volume(twist)
            new, records = device_rigid.rigid_run_3d(
                reference, depth, code, self.camera, self.array_offset, self.rigid_iterations, self.rigid_rate,
                self.eta, self.voxel_size, self.voxel_size, self.narrow_band_width_voxels, twist=twist)
            return Tracked(new, [unpack_rigid_record(r) for r in records], hits, True)  # the prediction's volume goes
        return Tracked(twist, [], None, False)

    def _track_judged(self, depth, code, last_good, colour_image, coarse):
        """a frame k >= 1 under a tracking_quality (package docstring, "Tracking quality and relocalisation"): tracked
        from the last good twist unless the state is lost, judged, and with a relocaliser tried again from the nearest
        keyframes' twists and last from the last good twist.  Returns the Tracked of the attempt that was good -- of
        the last attempt, with the last good twist, when none was --, whether the frame is fused, and the verdict: a
        dict of state, quality and, with a relocaliser that was asked, relocalisation"""
        tracker = self.icp if self.tracking_reference == "icp" else self.sdf_tracker
        shape = tuple(depth.shape)

        def attempt(start):
            tracked = self._track(depth, code, start.copy(), colour_image)
            last = tracked.records[-1] if tracked.records else None
            stride = 1 if last is None else level_stride(tracker, last["level"])
            return tracked, self.tracking_quality.judge(last, shape, stride)

        reloc = self.relocaliser
        was_lost = reloc is not None and self.tracking_state == "lost"
        tracked, quality, state, verdict = None, None, "lost", {}
        if not was_lost:
            tracked, quality = attempt(last_good)
            if quality["good"]:
                state = "tracking"
        if state == "lost" and reloc is not None:
            found = reloc.query(coarse)
            verdict["relocalisation"] = {"candidates": found["nearest"], "distances": found["distances"],
                                         "chosen": None}
            starts = [(i, reloc.twists[i]) for i in found["nearest"]] + ([(-1, last_good)] if was_lost else [])
            for chosen, start in starts:  # the last good twist last; a frame that just failed from it is not tried again
                tracked, quality = attempt(start)
                if quality["good"]:
                    state = "relocalised"
                    verdict["relocalisation"]["chosen"] = chosen
                    self._recovering = reloc.resume_after
                    break
        good = fuse = state != "lost"
        if good and self._recovering > 0:  # tracked, not fused: the model waits until the track has settled
            self._recovering -= 1
            fuse = False
            state = state if state == "relocalised" else "recovering"
        verdict["state"], verdict["quality"] = state, {k: quality[k] for k in ("pair_fraction", "rms", "skipped")}
        return (tracked if good else tracked._replace(twist=last_good)), fuse, verdict

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

    def _register(self, depth_image, colour_image):
        """with a sensor the raw pair becomes the registered pair, and everything after it sees that stream: the
        frame's (depth_image, colour_image, device registration record or None)"""
        if self.sensor is None:
            return depth_image, colour_image, None
        return self.sensor.register_device(depth_image, colour_image)

    def _track_frame(self, k, depth, code, colour_image, coarse):
        """frame k's (Tracked, whether it is fused, verdict): frame 0 takes the initial twist, a later frame is tracked
        from the last twist, under a tracking_quality by _track_judged; the verdict is empty without a judgement"""
        if k == 0:
            return Tracked(self.initial_twist.copy(), [], None, False), True, {}
        if self.tracking_quality is not None:
            return self._track_judged(depth, code, self.twists[-1].copy(), colour_image, coarse)
        return self._track(depth, code, self.twists[-1].copy(), colour_image), True, {}

    def _nonrigid_step(self, depth, code, twist):
        """the frame's live volume under twist through the non-rigid optimizer.  A warped step sets `warp` and drops
        the live volume before it returns None: the frame is fused through the field, in depth mode.  The volume-mode
        step returns the live volume, warped in place into the model, for integrate_volume"""
        model, optimizer = self.canonical, self.nonrigid_optimizer
        live = device_rigid.live_volume_3d(depth, code, self.camera, self.field_shape, self.array_offset, twist,
                                           **self._gen)
        if self._composed:
            optimizer.optimize(live, model.tsdf)
            self.warp = optimizer.cumulative_warp_field
        elif self.warped:
            self.warp = optimizer.optimize(model.tsdf, live)
        else:
            optimizer.optimize(live, model.tsdf)
            return live
        return None

    def _fuse(self, depth, code, colour_image, tracked, live, warp):
        """the frame fused into the model, and its unpacked record (the frame's host wait): in volume mode `live`, the
        non-rigid step's live volume; in depth mode the depth image under the tracked twist, through `warp` when the
        frame has one"""
        model = self.canonical
        if live is not None:
            return unpack_record(device_fusion.integrate_volume(model.tsdf, model.weight, live, 1.0,
                                                                model.max_weight).cpu().numpy())
        record, unpack = device_fusion.integrate_depth_by_arguments(
            model.tsdf, model.weight, depth, code, self.camera, self.array_offset, tracked.twist, w=1.0,
            max_weight=model.max_weight, pixel_weight=self._frame_weight(depth, code, tracked.ran), carve=self.carve,
            colour=model.colour, colour_image=device_colour_image(colour_image) if self.colour else None,
            colour_band=self.colour_band, warp=warp, **self._gen)
        return unpack(record.cpu().numpy())

    def _judgement_entries(self, frame, verdict, fuse, coarse):
        """what a tracking_quality and a relocaliser add to the frame record; every fused frame may become a
        keyframe"""
        if self.tracking_quality is not None:
            frame["tracking_state"] = self.tracking_state = verdict.get("state", "tracking")
            frame["tracking_quality"] = verdict.get("quality")
        if self.relocaliser is not None:
            frame["relocalisation"] = verdict.get("relocalisation")
            frame["keyframe"] = None
            if fuse:
                frame["keyframe"] = self.relocaliser.query(coarse, harvest=True, twist=frame["twist"])["appended"]

    def _shift_window(self, frame):
        """between frames, with a moving_volume: the policy reads the frame's twist, already on the host, the window
        moves, and the frame record gains shift, streamed_faces and, with a brick store, bricks_out and bricks_in"""
        mv = self.moving_volume
        s = mv.shift_for(frame["twist"], self.array_offset, self.field_shape, self.voxel_size)
        self.array_offset, chunks = self.canonical.shift(s, self.array_offset, self.voxel_size, mv.stream_mesh,
                                                         mv.min_weight, mv.normals,
                                                         colours=mv.stream_mesh and self.colour,
                                                         brick_store=self.brick_store)
        self.streamed_meshes.extend(chunks)
        frame["shift"] = s
        frame["streamed_faces"] = int(sum(len(c[1]) for c in chunks))
        if self.brick_store is not None:
            frame["bricks_out"] = self.brick_store.last["bricks_out"]
            frame["bricks_in"] = self.brick_store.last["bricks_in"]

    def integrate(self, depth_image, colour_image=None):
        """track and fuse one frame; returns its record (also appended to frame_records).  A sequence made with
        colour=True needs the frame's colour_image (uint8 (H, W, 3), numpy or device), any other takes none"""
        if self.colour and colour_image is None:
            raise ValueError("a sequence made with colour=True needs a colour_image on every frame")
        if not self.colour and colour_image is not None:
            raise ValueError("colour_image needs a sequence made with colour=True")
        k = len(self.twists)
        depth_image, colour_image, registration = self._register(depth_image, colour_image)
        depth, code = device_depth(depth_image)
        sdf_joint = self.sdf_tracker is not None and self.sdf_tracker.photometric_weight is not None
        if self.photometric_weight is not None or sdf_joint:
            colour_image = device_colour_image(colour_image)  # once: the tracker and the fusion both read it
        coarse = None
        if self.relocaliser is not None:
            coarse = self.relocaliser.encode(depth, self.camera, colour_image if self.colour else None)
        tracked, fuse, verdict = self._track_frame(k, depth, code, colour_image, coarse)
        through = self.nonrigid_optimizer is not None and k > 0 and fuse  # the frame takes the non-rigid step
        live = self._nonrigid_step(depth, code, tracked.twist) if through else None
        fusion = None  # a frame that is not good leaves the model alone
        if fuse:
            fusion = self._fuse(depth, code, colour_image, tracked, live, self.warp if through else None)
        del live
        frame = {"frame": k, "twist": np.asarray(tracked.twist, dtype=np.float64).reshape(6).copy(),
                 "rigid_records": tracked.records,
                 "nonrigid": self.nonrigid_optimizer.engine.last_call if through else None, "fusion": fusion,
                 "prediction_hits": None if tracked.hits is None else int(tracked.hits.item())}
        self._judgement_entries(frame, verdict, fuse, coarse)
        if registration is not None:
            frame["registration"] = device_rgbd.unpack_record(registration.cpu().numpy())
        if self.moving_volume is not None:
            self._shift_window(frame)
        if self.tracking_reference == "raycast":
            self._previous = (depth, code)
        self.twists.append(frame["twist"].copy())
        self.frame_records.append(frame)
        return frame

    def extract_mesh(self, iso=0.0, min_weight=0.0, normals=False, as_tensor=False, colours=False,
                     default_colour=device_mesh.DEFAULT_COLOUR, include_streamed=False, simplify_cell=None, weld=False,
                     min_component_faces=None, keep_largest_components=None, smooth_iterations=None,
                     smooth_boundary="fixed"):
        """CanonicalVolume.extract_mesh of the model with the sequence's array_offset and voxel_size.  With
        include_streamed (a sequence made with a moving_volume that streams) the window's mesh is followed by the
        streamed chunks, merge_meshes of them all: host arrays only, and only as the chunks were made -- iso 0, the
        policy's min_weight and normals, colours exactly when the sequence has colour, the default default_colour;
        anything else raises, since the chunks cannot be drawn again.  With a moving_volume that has keep_tsdf,
        include_streamed meshes CanonicalVolume.assemble of the window and the brick store instead: one mesh of the
        whole map without seams, at the caller's iso, min_weight, normals and colours, as tensors too.
        simplify_cell (metres, lattice through the world origin) clusters the result's vertices, on every path.  weld
        (only with include_streamed and a moving_volume that streams: nothing else has seams) first makes one vertex of
        the seam vertices that the merged chunks hold once each; `mesh_records` keeps the records of the last call,
        {"weld": ..., "simplify": ...}, None where a step did not run.  min_component_faces and
        keep_largest_components remove floaters last, after include_streamed, weld and simplify_cell, on every path
        (filter_mesh_components with min_faces and keep_largest); `mesh_records` then also has "components", that
        step's record.  An unwelded seam of streamed meshes splits a component in two, so with include_streamed on a
        moving_volume that streams meshes weld=True is what one wants with them.  smooth_iterations runs that many
        Taubin iterations (smooth_mesh with the default lambda and mu and boundary=smooth_boundary) after weld and
        simplify_cell and before the component filter, on every path, the normals rebuilt when the mesh has them;
        `mesh_records` then also has "smooth".  With "fixed" an unwelded seam stays bit for bit in place, so welding
        afterwards still closes it; welded first, the seam is smoothed like the rest."""
        self.mesh_records = dict(weld=None, simplify=None)
        floaters = dict(min_faces=min_component_faces, keep_largest=keep_largest_components)
        filtering = min_component_faces is not None or keep_largest_components is not None
        mv = self.moving_volume
        if weld and not (include_streamed and mv is not None and mv.stream_mesh):
            raise ValueError("weld=True needs include_streamed=True and a moving_volume that has stream_mesh=True: no "
                             "other mesh has seams")
        if not include_streamed:
            out = self.canonical.extract_mesh(self.array_offset, self.voxel_size, iso, min_weight, normals, as_tensor,
                                              colours, default_colour, simplify_cell, min_component_faces,
                                              keep_largest_components, smooth_iterations, smooth_boundary)
            record = self.canonical.mesh_record
            if filtering or smooth_iterations is not None:
                record = dict(record)  # the volume keeps its own
                for step in ("smooth", "components"):
                    if step in record:
                        self.mesh_records[step] = record.pop(step)
                record = record or None
            self.mesh_records["simplify"] = record
            return out
        if mv is not None and mv.keep_tsdf:
            if colours and not self.colour:
                raise ValueError("colours=True needs a sequence made with colour=True")
            tsdf, weight, colour, offset = self.canonical.assemble(self.brick_store, self.array_offset)
            out = device_mesh.extract_mesh(tsdf, weight, offset, self.voxel_size, iso, min_weight, normals,
                                           *((colour, default_colour) if colours else ()))
            out, self.mesh_records["simplify"] = simplified(out, normals, colours, simplify_cell)
            out, record = smoothed(out, normals, colours, smooth_iterations, smooth_boundary)
            if record is not None:
                self.mesh_records["smooth"] = record
            out, record = components_filtered(out, normals, colours, min_component_faces, keep_largest_components)
            if filtering:
                self.mesh_records["components"] = record
            return mesh_outputs(out, normals, colours, as_tensor)
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
        merged = merge_meshes([window] + self.streamed_meshes)
        if weld:
            *merged, self.mesh_records["weld"] = simplify_mesh(merged, return_record=True)
        if simplify_cell is not None:
            *merged, self.mesh_records["simplify"] = simplify_mesh(tuple(merged), simplify_cell, return_record=True)
        if smooth_iterations is not None:
            *merged, self.mesh_records["smooth"] = smooth_mesh(tuple(merged), smooth_iterations,
                                                               boundary=smooth_boundary, return_record=True)
        if filtering:
            *merged, self.mesh_records["components"] = filter_mesh_components(tuple(merged), return_record=True,
                                                                              **floaters)
        return tuple(merged)

    def esdf(self, max_distance_voxels=32, iso=0.0, min_weight=0.0, unknown="free", nearest=False, as_tensor=False,
             include_streamed=False):
        """CanonicalVolume.esdf of the model with the sequence's voxel_size: the Euclidean signed distance field in
        metres, or (esdf, nearest).  With include_streamed (a sequence made with a moving_volume that has keep_tsdf)
        it is the field of CanonicalVolume.assemble of the window and the brick store, the whole map, and
        `last_esdf_offset` is that box's array offset; without it `last_esdf_offset` is the window's array_offset.
        `last_esdf_record` is the call's record"""
        mv = self.moving_volume
        if include_streamed and (mv is None or not mv.keep_tsdf):
            raise ValueError("include_streamed needs a sequence made with a moving_volume that has keep_tsdf=True: only a "
                             "brick store keeps the values that left the window")
        store = dict(brick_store=self.brick_store, array_offset=self.array_offset) if include_streamed else {}
        out = self.canonical.esdf(self.voxel_size, max_distance_voxels, iso, min_weight, unknown, nearest, as_tensor,
                                  **store)
        self.last_esdf_record = self.canonical.last_esdf_record
        self.last_esdf_offset = self.canonical.last_esdf_offset if include_streamed else self.array_offset.copy()
        return out
