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
simplify_mesh(mesh, cell_size=None, origin=(0, 0, 0)) welds or decimates a mesh in that layout (INTEGRATION.md section 3,
"Mesh simplification"; tests/mesh_simplify_restatement.py restates it; csrc/lsf_mesh_simplify.hip): vertices are grouped
by a key -- the bit patterns of the position with -0 read as +0 (cell_size None: welding), or the cell
floor((p - origin) / cell_size) of a lattice, at most 2^20 cells from the origin (vertex clustering) -- and the groups
are numbered by their first member.  A group becomes one vertex: the first member's bits when welding, else the centre
of the members' 2^-24-cell quantisation bins, float32(origin + cell_size (c + (sum q + n / 2) / (n 2^24))), within
cell_size 2^-25 of their mean, so a cluster of one does not promise its member's bits back; its normal is the
normalised integer sum of the members' normals scaled by 2^30, its colour the rounded integer mean.  Faces are remapped;
one with two equal ids is dropped; the rest are grouped by their sorted ids, a face counting +1 when it is a rotation
of the sorted triple and -1 otherwise: a group whose signs cancel is dropped whole (a flap), any other keeps its first
face of the majority orientation.  Clusters no surviving face uses are removed.  Orders are the inputs' and every sum
is an integer sum, so the result does not depend on how the lanes ran: groups are found with a hash table claimed by
compare-and-swap, never by a sort.  A non-finite vertex or a face index outside the vertices raises ValueError after
the one host read, that of the 13-word record (return_record=True returns it).  merge_meshes(..., weld=True),
CanonicalVolume.extract_mesh(..., simplify_cell=) and SequenceFusion3d.extract_mesh(..., simplify_cell=, weld=) go
through it -- simplify_cell in metres on the lattice through the world origin; weld, with include_streamed and a window
that streams, makes one vertex of the seam vertices the merged chunks hold once each, before any clustering -- and
every keyword defaults to the call as it was.  Cost: profiles/mesh_simplify_cost.md.
mesh_components(mesh) labels the connected components of a mesh in that layout and filter_mesh_components(mesh,
min_faces=None, min_vertices=None, min_extent=None, keep_largest=None) removes the ones one does not want: the floaters
that noise, flying pixels and half-carved surfaces leave around a model fused from real depth (INTEGRATION.md section 3,
"Mesh components"; tests/mesh_components_restatement.py restates it; csrc/lsf_mesh_components.hip).  Two vertices are
connected when some face names both, and a component is a connected set of vertices; a degenerate face still connects
what it names, and a vertex that no face names is a component of its own with 0 faces.  A component's label is the
smallest vertex index in it and a face's label the label of its first vertex, so the answer is a function of the mesh
alone, not of the launch shape or of the order in which lanes ran.  mesh_components returns (vertex_labels int32 (V,),
face_labels int32 (F,), table), the table a dict of labels, vertex_counts, face_counts int32 (C,) and bounds float32
(C, 2, 3) for the C components in ascending label order; the bounds are the componentwise minimum and maximum of the
members' positions, exact, with -0 read as +0 as the weld does.  A component passes the filter when it meets every
threshold that is given -- face count >= min_faces, vertex count >= min_vertices, the longest edge of its bounds >=
min_extent, compared in float64 of the float32 bounds and so exactly --, and with keep_largest = k only the first k
passing components stay, in the order face count descending, label ascending.  Kept vertices and kept faces keep their
input order, faces are re-indexed, normals and colours are carried bit for bit; no criterion at all is a ValueError.  The
labels come from a lock-free union-find with integer atomics: a root is linked under a smaller index by
compare-and-swap, so every walk is strictly decreasing and the final root is the component's minimum; every loop ends
after V + 1 steps at the latest, and a lane that ever got there would raise RuntimeError through the record.  A face
index outside [0, V) or a non-finite vertex is counted on the card before any gather through it and raises ValueError
after the first host read; mesh_components reads the 9-word record once (the number of components), the filter twice
(then the sizes of its outputs; return_record=True returns it).  CanonicalVolume.extract_mesh(...,
min_component_faces=, keep_largest_components=) and the same keywords of SequenceFusion3d.extract_mesh apply the filter
last, after include_streamed, weld and simplify_cell, and add the record to mesh_record / mesh_records under
"components"; with both None the calls are as they were.  An unwelded seam of streamed meshes splits a component, so
weld=True is what one wants with them.  Cost: profiles/mesh_components_cost.md.
smooth_mesh(mesh, iterations=10, lam=0.5, mu=-0.53, boundary="fixed", recompute_normals=True) removes the surface noise
that marching cubes copies out of a TSDF fused from real depth, and mesh_vertex_normals(mesh) gives the area-weighted
vertex normals of any mesh in that layout from its faces alone ("Mesh smoothing";
tests/mesh_smooth_restatement.py restates it; csrc/lsf_mesh_smooth.hip).  An iteration is a pass with weight lam and,
unless mu is 0, a pass with weight mu: Taubin's lambda | mu, which keeps the volume that plain Laplacian passes (mu=0.0)
lose.  Edges: every face contributes its corner pairs (0,1), (1,2), (2,0); a pair with equal ends is skipped, every
other pair adds 1 to the face count of its undirected edge.  Two vertices are neighbours when an edge joins them; d(i)
is the number of distinct neighbours of vertex i.  With boundary="fixed" the ends of every edge whose face count is not
2 -- open borders, the seams of streamed chunks, non-manifold edges -- are pinned, with "free" none is; a pinned vertex
and a vertex with d = 0 keep their position bit for bit through every pass, so weld=True closes a seam after smoothing
as before.  One pass with weight w: B is the largest |coordinate| of the pass's input (an integer maximum on the float
bits), e = max(E, 1) - 126 with E the exponent field of B's bits, so that B < 2^e, q = 2^(e-32) and q = 1 when B = 0;
Q(x) = (int64) rint(double(x) / q), ties to even, 0 for a non-finite x; S_i is the sum of Q(p_j) over the neighbours,
per axis, in integers, so no order of the sum can matter; m = (double(S_i) * q) / double(d(i)); p_i' = float32(double(p_i)
+ w * (m - double(p_i))), every float64 operation rounded on its own.  Positions are float32 between passes and every
pass takes B from its own input.  Vertex count and order, faces and colours are unchanged; iterations=0 returns the
positions bit for bit.  Normals: every face (a, b, c) adds c = (p_b - p_a) x (p_c - p_a), computed in float64 and
quantised to (int64) rint(c / qn) with qn = 2^(em-32), M < 2^em the largest |component| of any face, to its three
vertices by integer atomics; the normal is float32(S / L) with L = sqrt((S_x^2 + S_y^2) + S_z^2), and (0, 0, 0) when L
= 0, which the record counts.  It is the right-hand normal, extract_mesh's "towards larger tsdf".  smooth_mesh rebuilds
the normals of a mesh that has them from the smoothed faces unless recompute_normals=False, which carries them bit for
bit.  The outputs equal the restatement bit for bit at any launch shape and table size.  ValueError before any launch:
iterations not a whole number in 0 .. 1000, lam not finite or outside (0, 1], mu not finite or > 0, a boundary other
than the two names, a layout that is none of extract_mesh's; after the one read of the 13-word record: a non-finite
vertex or a face index outside [0, V) (return_record=True reads the record a second time and returns it).
CanonicalVolume.extract_mesh(..., smooth_iterations=, smooth_boundary="fixed") and the same keywords of
SequenceFusion3d.extract_mesh smooth with the default lambda and mu after simplify_cell / weld and before the component
filter, which stays last, rebuild the normals with normals=True and add the record to mesh_record / mesh_records under
"smooth"; with None the calls are as they were.  Cost: profiles/mesh_smooth_cost.md.
CanonicalVolume.esdf(voxel_size, max_distance_voxels=32, iso=0, min_weight=0, unknown="free", nearest=False) answers
"how far is this voxel from the nearest surface?", which the model's own values do not: they are projective distances
along the pixel's ray, truncated at +-1 ("Euclidean distance field";
tests/esdf_restatement.py restates it; csrc/lsf_esdf.hip).  A voxel is observed when weight > min_weight and inside when
it is observed with tsdf < iso; a site is an observed voxel with an in-bounds observed 6-neighbour of the other inside
flag, so both sides of every zero crossing between observed voxels are sites, and with unknown="occupied" every voxel
that is not observed is a site too.  key(v) = min over the sites s of (|v - s|^2, flat(s)), lexicographic, with the
integer squared lattice distance and flat(s) = (z Y + y) X + x: ties go to the smallest flat index, so the result is a
function of the inputs alone.  distance2 is the key's first part where it is <= max_distance_voxels^2 (inclusive), else
2^31 - 1; nearest its second part, else -1; esdf = sign * (sqrtf(float(distance2)) * float(voxel_size)) in metres, with
float(max_distance_voxels) in place of the root beyond the cap, sign -1 where the voxel is inside and +1 elsewhere --
also where it was never observed under unknown="free": `weight` masks those if the caller wants that.  The key is
separable, so the kernels are a pass along x (which also finds the sites), one along y and one along z, integers
throughout, and equal the restatement's brute force exactly.  A model without a site gives the cap everywhere and is
no error.  `last_esdf_record` keeps {"sites", "finite", "max_distance2"}; brick_store= / array_offset= give the field
of assemble()'s whole map, and SequenceFusion3d.esdf(include_streamed=True) passes its own.  One host synchronisation,
the read of the record.  Cost: profiles/esdf_cost.md.

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
chunks.  Every cell is drawn exactly once; the vertices on a seam appear on both sides (weld=True makes one of
those whose bits agree: simplify_mesh above), and since the window goes on
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
vertex and face totals; simplify_cell= and weld= add one each, the read of the simplification's record, min_component_faces= /
keep_largest_components= two, the reads of the components' record, smooth_iterations= one, the read of the smoothing's
record.  A moving
volume's policy adds none (the twist is on the host already); a shift that streams
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
colours, for mesh simplification quadric-error placement of the new vertices, a target face count, welding within a
tolerance across seams that later frames have moved and per-face attributes, for mesh smoothing cotangent weights, bilateral or
feature-preserving smoothing, a user pin mask and smoothing the TSDF itself, for mesh components edge-adjacency
instead of vertex-adjacency, per-component area or volume and components of the volume itself, a mesh extracted without the host read of
its totals, for the Euclidean distance field an incremental update after a fusion or a shift, a 2-D slice call,
sub-voxel site positions, z-slab and multi-GPU volumes and feeding the trackers or the level-set term from the field,
for the
relocaliser relocalising inside a moving window, saving the keyframe database, loop closure and a learned quality
test, and for the moving volume a shift enqueued without the mesh totals' host read, and for its
brick store saving the store to disk, streaming without the host read of the brick total, and bricks in half
precision."""
from ..device_esdf import RECORD_FIELDS as ESDF_RECORD_FIELDS, unpack_record as unpack_esdf_record
from ..device_fusion import (COLOUR_RECORD_FIELDS, RECORD_FIELDS, WARPED_RECORD_FIELDS, WEIGHTED_RECORD_FIELDS,
                             unpack_colour_record, unpack_record, unpack_warped_record, unpack_weighted_record)
from .brick_store import BrickStore
from .canonical_volume import CanonicalVolume
from .depth_confidence import DepthConfidence
from .mesh_components import filter_mesh_components, mesh_components
from .mesh_simplify import simplify_mesh
from .mesh_smooth import mesh_vertex_normals, smooth_mesh
from .moving_volume import MovingVolume, merge_meshes
from .relocaliser import Relocaliser, TrackingQuality
from .rgbd_sensor import RgbdSensor
from .sequence import DIRECT_TRACKING_MODES, TRACKING_MODES, TRACKING_REFERENCES, SequenceFusion3d

__all__ = ["CanonicalVolume", "SequenceFusion3d", "DepthConfidence", "MovingVolume", "BrickStore", "RgbdSensor",
           "Relocaliser", "TrackingQuality",
           "merge_meshes", "simplify_mesh", "mesh_components", "filter_mesh_components",
           "smooth_mesh", "mesh_vertex_normals",
           "unpack_record", "unpack_weighted_record",
           "unpack_colour_record", "unpack_warped_record", "RECORD_FIELDS", "WEIGHTED_RECORD_FIELDS",
           "COLOUR_RECORD_FIELDS", "WARPED_RECORD_FIELDS", "ESDF_RECORD_FIELDS", "unpack_esdf_record",
           "TRACKING_REFERENCES", "TRACKING_MODES", "DIRECT_TRACKING_MODES"]
