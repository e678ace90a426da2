"""ctypes mirror of include/take_hip.h (field order and types must match the header)."""
import ctypes as C

c_double3 = C.c_double * 3
c_double4 = C.c_double * 4
c_float3 = C.c_float * 3

TAKE_PRECISION_F32 = 0
TAKE_PRECISION_F64 = 1
TAKE_PRECISION_MIXED = 2  # first exact_bounces rounds in f64, the rest in f32; records and images are f64
TAKE_OK, TAKE_E_INVALID, TAKE_E_DEVICE, TAKE_E_NO_GPU, TAKE_E_NOMEM = 0, -1, -2, -3, -4

MAT_DIFFUSE, MAT_MIRROR, MAT_PLASTIC, MAT_PHONG, MAT_BLINN_PHONG, MAT_BLINN_PHONG_MICROFACET = range(6)
MAT_DISNEY_DIFFUSE, MAT_DISNEY_METAL, MAT_DISNEY_GLASS, MAT_DISNEY_CLEARCOAT, MAT_DISNEY_SHEEN, MAT_DISNEY_BSDF = range(6, 12)
# extension (tags of the real lobes; include/take_hip.h): the Disney tag + 5
MAT_BURLEY_METAL, MAT_BURLEY_GLASS, MAT_BURLEY_CLEARCOAT, MAT_BURLEY_SHEEN, MAT_BURLEY_BSDF = range(12, 17)
MATERIAL_PARAMS = 12


class TakeTexture(C.Structure):
    _fields_ = [("kind", C.c_int32), ("image_id", C.c_int32), ("value", c_double3),
                ("uscale", C.c_double), ("vscale", C.c_double), ("uoffset", C.c_double), ("voffset", C.c_double)]


class TakeMaterial(C.Structure):
    _fields_ = [("tag", C.c_int32), ("reserved", C.c_int32), ("reflectance", TakeTexture), ("param", C.c_double * 12)]


class TakeImage3(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("data", C.POINTER(C.c_double))]


class TakeMesh(C.Structure):
    _fields_ = [("n_vertices", C.c_int64), ("n_faces", C.c_int64), ("positions", C.POINTER(C.c_double)),
                ("indices", C.POINTER(C.c_int32)), ("normals", C.POINTER(C.c_double)), ("uvs", C.POINTER(C.c_double)),
                ("material_id", C.c_int32), ("flags", C.c_int32)]


TAKE_MESH_DEVICE_ARRAYS = 1


class TakePlyLayout(C.Structure):
    _fields_ = [("n_vertices", C.c_int64), ("n_faces", C.c_int64), ("vertex_offset", C.c_int64), ("face_offset", C.c_int64),
                ("vertex_stride", C.c_int32), ("face_stride", C.c_int32), ("has_normals", C.c_int32), ("has_uvs", C.c_int32),
                ("position_is_f64", C.c_int32), ("index_bytes", C.c_int32), ("header_bytes", C.c_int32), ("reserved", C.c_int32)]


# mesh ingest on the device, and the normals of host arrays (include/take_hip.h): name -> argument types
MESH_PROTOTYPES = {
    "take_hip_ply_layout": [C.c_void_p, C.c_size_t, C.POINTER(TakePlyLayout)],
    "take_hip_mesh_from_ply": [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(TakeMesh)],
    "take_hip_mesh_from_ply_file": [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(TakeMesh)],
    "take_hip_mesh_from_serialized": [C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(TakeMesh)],
    "take_hip_mesh_from_serialized_file": [C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(TakeMesh)],
    "take_hip_mesh_from_obj": [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(TakeMesh)],
    "take_hip_mesh_from_obj_file": [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(TakeMesh)],
    "take_hip_mesh_download": [C.POINTER(TakeMesh), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "take_hip_mesh_release": [C.POINTER(TakeMesh)],
    "take_hip_mesh_compute_normals": [C.POINTER(TakeMesh)],
    "take_hip_compute_normals": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p],
}


class TakeSphere(C.Structure):
    _fields_ = [("center", c_double3), ("radius", C.c_double), ("material_id", C.c_int32), ("reserved", C.c_int32)]


class TakeLight(C.Structure):
    _fields_ = [("kind", C.c_int32), ("shape_id", C.c_int32), ("intensity", c_double3), ("position", c_double3)]


class TakeInstance(C.Structure):
    _fields_ = [("mesh_id", C.c_int32), ("material_id", C.c_int32), ("xform", C.c_double * 12)]


class TakeCamera(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("lookfrom", c_double3), ("lookat", c_double3),
                ("up", c_double3), ("vfov", C.c_double)]


class TakeSceneDesc(C.Structure):
    _fields_ = [("camera", TakeCamera), ("background", c_double3),
                ("n_meshes", C.c_int32), ("n_spheres", C.c_int32),
                ("meshes", C.POINTER(TakeMesh)), ("spheres", C.POINTER(TakeSphere)),
                ("n_shapes", C.c_int64),
                ("shape_kind", C.POINTER(C.c_int32)), ("shape_ref", C.POINTER(C.c_int32)),
                ("shape_face", C.POINTER(C.c_int32)), ("shape_area_light", C.POINTER(C.c_int32)),
                ("n_lights", C.c_int32), ("n_materials", C.c_int32),
                ("lights", C.POINTER(TakeLight)), ("materials", C.POINTER(TakeMaterial)),
                ("n_images", C.c_int32), ("reserved", C.c_int32), ("images", C.POINTER(TakeImage3)),
                ("n_instances", C.c_int64), ("instances", C.POINTER(TakeInstance))]


class TakeBuildOpts(C.Structure):
    _fields_ = [("precision", C.c_int32), ("bvh_threads", C.c_int32), ("max_leaf_size", C.c_int32),
                ("builder", C.c_int32), ("burley_lobes", C.c_int32), ("instances", C.c_int32)]


TAKE_INSTANCES_TWO_LEVEL = 0    # placements are leaves of a top-level BVH
TAKE_INSTANCES_FLATTEN = 1      # placements expanded to world-space triangles by scene_create
TAKE_BUILDER_AUTO = 0          # host SAH below 4M shapes, device LBVH from there on
TAKE_BUILDER_DEVICE_LBVH = 1
TAKE_BUILDER_HOST_SAH = 2


# prototypes of the entry points that change a resident scene (include/take_hip.h): name -> argument types
class TakeMeshUpdate(C.Structure):
    """take_hip_scene_set_mesh_vertices: new arrays of one mesh (host memory, or device memory under TAKE_MESH_DEVICE_ARRAYS)"""
    _fields_ = [("mesh", C.c_int32), ("flags", C.c_int32), ("positions", C.c_void_p), ("normals", C.c_void_p)]


SCENE_UPDATE_PROTOTYPES = {
    "take_hip_scene_set_instance_transforms": [C.c_void_p, C.c_void_p, C.c_int64],
    "take_hip_scene_set_instance_transforms_device": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "take_hip_scene_set_camera": [C.c_void_p, C.POINTER(TakeCamera)],
    "take_hip_scene_set_mesh_vertices": [C.c_void_p, C.POINTER(TakeMeshUpdate), C.c_int32],
    "take_hip_scene_update_meshes": [C.c_void_p, C.POINTER(TakeMeshUpdate), C.c_int32],
}


# rigs: skinning and morph targets on the device (include/take_hip.h: take_hip_rig_*, take_hip_scene_pose_meshes)
TAKE_RIG_DEVICE_ARRAYS = 1
TAKE_RIG_POSE_DEVICE_ARRAYS = 1


class TakeRigDesc(C.Structure):
    """take_hip_rig_create: rest pose, influences and morph targets of one mesh (host memory, or device memory under
    TAKE_RIG_DEVICE_ARRAYS)"""
    _fields_ = [("n_vertices", C.c_int64), ("positions", C.c_void_p), ("normals", C.c_void_p), ("n_joints", C.c_int32),
                ("n_influences", C.c_int32), ("joints", C.c_void_p), ("weights", C.c_void_p), ("inverse_bind", C.c_void_p),
                ("n_targets", C.c_int32), ("target_positions", C.c_void_p), ("target_normals", C.c_void_p), ("flags", C.c_int32)]


class TakeRigPose(C.Structure):
    """one pose of a rig: n_joints x 12 joint -> world matrices and T target weights (host memory, or device memory under
    TAKE_RIG_POSE_DEVICE_ARRAYS)"""
    _fields_ = [("joint_xforms", C.c_void_p), ("target_weights", C.c_void_p), ("flags", C.c_int32)]


class TakeRigBinding(C.Structure):
    """take_hip_scene_pose_meshes: one mesh of the scene, the rig that poses it, the pose"""
    _fields_ = [("mesh", C.c_int32), ("reserved", C.c_int32), ("rig", C.c_void_p), ("pose", TakeRigPose)]


RIG_PROTOTYPES = {
    "take_hip_rig_create": [C.POINTER(TakeRigDesc), C.POINTER(C.c_void_p)],
    "take_hip_rig_destroy": [C.c_void_p],
    "take_hip_rig_info": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                          C.POINTER(C.c_int64)],
    "take_hip_rig_pose_device": [C.c_void_p, C.POINTER(TakeRigPose), C.c_void_p, C.c_void_p, C.c_void_p],
    "take_hip_rig_pose": [C.c_void_p, C.POINTER(TakeRigPose), C.c_void_p, C.c_void_p],
    "take_hip_scene_pose_meshes": [C.c_void_p, C.POINTER(TakeRigBinding), C.c_int32],
}


class TakeSubdivDesc(C.Structure):
    """take_hip_subdiv_create / _counts / _topology: a cage's topology (host memory) and the level count"""
    _fields_ = [("n_vertices", C.c_int64), ("n_faces", C.c_int64), ("indices", C.c_void_p), ("uvs", C.c_void_p), ("levels", C.c_int32), ("flags", C.c_int32)]


class TakeSubdivBinding(C.Structure):
    """take_hip_scene_subdivide_meshes: one mesh of the scene, the handle that refines it, the cage — positions, or a
    rig and its pose"""
    _fields_ = [("mesh", C.c_int32), ("flags", C.c_int32), ("subdiv", C.c_void_p), ("cage_positions", C.c_void_p), ("rig", C.c_void_p), ("pose", TakeRigPose)]


TAKE_SUBDIV_DEVICE_ARRAYS = 1
SUBDIV_PROTOTYPES = {
    "take_hip_subdiv_counts": [C.POINTER(TakeSubdivDesc), C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "take_hip_subdiv_topology": [C.POINTER(TakeSubdivDesc), C.c_void_p, C.c_void_p],
    "take_hip_subdiv_create": [C.POINTER(TakeSubdivDesc), C.POINTER(C.c_void_p)],
    "take_hip_subdiv_destroy": [C.c_void_p],
    "take_hip_subdiv_info": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)],
    "take_hip_subdiv_refine_device": [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "take_hip_subdiv_refine": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "take_hip_scene_subdivide_meshes": [C.c_void_p, C.POINTER(TakeSubdivBinding), C.c_int32],
}


class TakeDisplaceDesc(C.Structure):
    """take_hip_displace_create: a mesh's topology and uvs (host memory), a one-channel height image (host memory, or
    device memory under TAKE_DISPLACE_DEVICE_ARRAYS) and the lookup"""
    _fields_ = [("n_vertices", C.c_int64), ("n_faces", C.c_int64), ("indices", C.c_void_p), ("uvs", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("texels", C.c_void_p), ("real", C.c_int32), ("flags", C.c_int32), ("uscale", C.c_double), ("vscale", C.c_double), ("uoffset", C.c_double),
                ("voffset", C.c_double)]


class TakeDisplaceBinding(C.Structure):
    """take_hip_scene_displace_meshes: one mesh of the scene, the handle that displaces it, the amplitude, the base
    surface — positions and optional normals, or a subdivision handle with its cage (positions, or a rig and its pose)"""
    _fields_ = [("mesh", C.c_int32), ("flags", C.c_int32), ("displace", C.c_void_p), ("scale", C.c_double), ("bias", C.c_double), ("positions", C.c_void_p),
                ("normals", C.c_void_p), ("subdiv", C.c_void_p), ("cage_positions", C.c_void_p), ("rig", C.c_void_p), ("pose", TakeRigPose)]


TAKE_DISPLACE_DEVICE_ARRAYS = 1
DISPLACE_PROTOTYPES = {
    "take_hip_displace_create": [C.POINTER(TakeDisplaceDesc), C.POINTER(C.c_void_p)],
    "take_hip_displace_destroy": [C.c_void_p],
    "take_hip_displace_info": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)],
    "take_hip_displace_apply_device": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p],
    "take_hip_displace_apply": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p],
    "take_hip_scene_displace_meshes": [C.c_void_p, C.POINTER(TakeDisplaceBinding), C.c_int32],
}


class TakeRenderOpts(C.Structure):
    _fields_ = [("spp", C.c_int32), ("max_depth", C.c_int32), ("seed", C.c_uint64), ("ray_epsilon", C.c_double),
                ("strip_first", C.c_int32), ("strip_stride", C.c_int32), ("samples_per_batch", C.c_int32),
                ("integrator", C.c_int32), ("exact_bounces", C.c_int32), ("reserved", C.c_int32)]


class TakeFeatureBuffers(C.Structure):
    """take_hip_render_features*: one pointer per plane (host or device memory), None = not wanted"""
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("alpha", C.c_void_p),
                ("shape_id", C.c_void_p), ("material_id", C.c_void_p)]


# the planes in the struct's order: name -> (values per pixel, True = the scene's Real / False = int32)
FEATURE_PLANES = {"albedo": (3, True), "normal": (3, True), "depth": (1, True), "alpha": (1, True),
                  "shape_id": (1, False), "material_id": (1, False)}

FEATURE_PROTOTYPES = {
    "take_hip_render_features_device": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeFeatureBuffers), C.c_void_p],
    "take_hip_render_features": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeFeatureBuffers)],
}


class TakeDenoiseOpts(C.Structure):
    """take_hip_denoise*: a field <= 0 takes its default (iterations 5, sigma_color 1.0, sigma_normal 0.3, sigma_depth
    0.05, albedo_floor 1e-3)"""
    _fields_ = [("iterations", C.c_int32), ("flags", C.c_int32), ("sigma_color", C.c_double), ("sigma_normal", C.c_double),
                ("sigma_depth", C.c_double), ("albedo_floor", C.c_double)]


TAKE_DENOISE_KEEP_ALBEDO = 1  # filter rgb as it is even when an albedo is given
DENOISE_DEFAULTS = {"iterations": 5, "sigma_color": 1.0, "sigma_normal": 0.3, "sigma_depth": 0.05, "albedo_floor": 1e-3}

# the image-space denoiser (include/take_hip.h): name -> argument types
DENOISE_PROTOTYPES = {
    "take_hip_denoise_device": [C.c_void_p, C.POINTER(TakeFeatureBuffers), C.c_int32, C.c_int32, C.c_int32,
                                C.POINTER(TakeDenoiseOpts), C.c_void_p, C.c_void_p],
    "take_hip_denoise": [C.c_void_p, C.POINTER(TakeFeatureBuffers), C.c_int32, C.c_int32, C.c_int32,
                         C.POINTER(TakeDenoiseOpts), C.c_void_p],
    "take_hip_render_denoised_device": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeDenoiseOpts), C.c_void_p, C.c_void_p],
    "take_hip_render_denoised": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeDenoiseOpts), C.c_void_p],
}


def denoise_opts(iterations=0, keep_albedo=False, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, albedo_floor=0.0):
    """-> TakeDenoiseOpts; what is left out takes the library's default"""
    return TakeDenoiseOpts(int(iterations), TAKE_DENOISE_KEEP_ALBEDO if keep_albedo else 0, float(sigma_color), float(sigma_normal),
                           float(sigma_depth), float(albedo_floor))


class TakeAdaptiveOpts(C.Structure):
    """take_hip_render_adaptive*: a field that is not positive takes its default (min_spp 16, step_spp 8, floor 1e-3);
    threshold < 0 takes 0.05 and 0 is a value"""
    _fields_ = [("min_spp", C.c_int32), ("step_spp", C.c_int32), ("threshold", C.c_double), ("floor", C.c_double),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class TakeAdaptiveStats(C.Structure):
    """take_hip_render_adaptive*: one pointer per plane (host or device memory), None = not wanted"""
    _fields_ = [("count", C.c_void_p), ("m1", C.c_void_p), ("m2", C.c_void_p)]


ADAPTIVE_DEFAULTS = {"min_spp": 16, "step_spp": 8, "threshold": 0.05, "floor": 1e-3}

# adaptive sampling (include/take_hip.h): name -> argument types
ADAPTIVE_PROTOTYPES = {
    "take_hip_render_adaptive_device": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeAdaptiveOpts), C.c_void_p,
                                        C.POINTER(TakeAdaptiveStats), C.c_void_p],
    "take_hip_render_adaptive": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeAdaptiveOpts), C.c_void_p, C.POINTER(TakeAdaptiveStats)],
}


def adaptive_opts(min_spp=0, step_spp=0, threshold=-1.0, floor=0.0):
    """-> TakeAdaptiveOpts; what is left out takes the library's default"""
    return TakeAdaptiveOpts(int(min_spp), int(step_spp), float(threshold), float(floor), 0, 0)


# the variance-guided denoiser (include/take_hip.h): TakeDenoiseOpts, but sigma_color counts the pixel's standard deviations
DENOISE_VARIANCE_DEFAULTS = dict(DENOISE_DEFAULTS, sigma_color=4.0)

# name -> argument types
DENOISE_VARIANCE_PROTOTYPES = {
    "take_hip_denoise_variance_device": [C.c_void_p, C.POINTER(TakeFeatureBuffers), C.POINTER(TakeAdaptiveStats), C.c_int32, C.c_int32, C.c_int32,
                                         C.POINTER(TakeDenoiseOpts), C.c_void_p, C.c_void_p, C.c_void_p],
    "take_hip_denoise_variance": [C.c_void_p, C.POINTER(TakeFeatureBuffers), C.POINTER(TakeAdaptiveStats), C.c_int32, C.c_int32, C.c_int32,
                                  C.POINTER(TakeDenoiseOpts), C.c_void_p, C.c_void_p],
    "take_hip_render_adaptive_denoised_device": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeAdaptiveOpts), C.POINTER(TakeDenoiseOpts), C.c_void_p,
                                                 C.POINTER(TakeAdaptiveStats), C.c_void_p, C.c_void_p],
    "take_hip_render_adaptive_denoised": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeAdaptiveOpts), C.POINTER(TakeDenoiseOpts), C.c_void_p,
                                          C.POINTER(TakeAdaptiveStats), C.c_void_p],
}


class TakeMotionBuffers(C.Structure):
    """take_hip_render_motion*: one pointer per plane (host or device memory), None = not wanted"""
    _fields_ = [("prev_xy", C.c_void_p), ("prev_depth", C.c_void_p), ("depth", C.c_void_p), ("shape_id", C.c_void_p)]


# name -> (values per pixel, True = the scene's Real / False = int32)
MOTION_PLANES = {"prev_xy": (2, True), "prev_depth": (1, True), "depth": (1, True), "shape_id": (1, False)}


class TakeTemporalFrame(C.Structure):
    """take_hip_temporal_accumulate*: one frame's planes (host or device memory); depth and shape_id may be None"""
    _fields_ = [("rgb", C.c_void_p), ("count", C.c_void_p), ("m1", C.c_void_p), ("m2", C.c_void_p), ("depth", C.c_void_p), ("shape_id", C.c_void_p)]


class TakeTemporalOpts(C.Structure):
    """a field that is not positive takes its default (max_history 64, depth_tol 0.05); flags: 0"""
    _fields_ = [("max_history", C.c_int32), ("flags", C.c_int32), ("depth_tol", C.c_double)]


TEMPORAL_DEFAULTS = {"max_history": 64, "depth_tol": 0.05}


def temporal_opts(max_history=0, depth_tol=0.0):
    """-> TakeTemporalOpts; what is left out takes the library's default"""
    return TakeTemporalOpts(int(max_history), 0, float(depth_tol))


# temporal reprojection and accumulation (include/take_hip.h): name -> argument types
TEMPORAL_PROTOTYPES = {
    "take_hip_scene_mark_frame": [C.c_void_p],
    "take_hip_render_motion_device": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeMotionBuffers), C.c_void_p],
    "take_hip_render_motion": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeMotionBuffers)],
    "take_hip_temporal_accumulate_device": [C.POINTER(TakeTemporalFrame), C.POINTER(TakeTemporalFrame), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                            C.POINTER(TakeTemporalOpts), C.POINTER(TakeTemporalFrame), C.c_void_p],
    "take_hip_temporal_accumulate": [C.POINTER(TakeTemporalFrame), C.POINTER(TakeTemporalFrame), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                     C.POINTER(TakeTemporalOpts), C.POINTER(TakeTemporalFrame)],
    "take_hip_render_temporal_device": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeAdaptiveOpts), C.POINTER(TakeTemporalOpts), C.POINTER(TakeDenoiseOpts),
                                        C.c_int32, C.c_void_p, C.c_void_p],
    "take_hip_render_temporal": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeAdaptiveOpts), C.POINTER(TakeTemporalOpts), C.POINTER(TakeDenoiseOpts),
                                 C.c_int32, C.c_void_p],
}

# following moved vertices in the motion pass (include/take_hip.h): name -> argument types
TAKE_TRACK_VERTICES = 1
TRACKING_PROTOTYPES = {
    "take_hip_scene_track_vertices": [C.c_void_p, C.c_int32],
    "take_hip_scene_tracking_info": [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)],
}


# the thin-lens camera (include/take_hip.h)
class TakeLens(C.Structure):
    """take_hip_scene_set_lens: aperture_radius 0 = pinhole; focus_distance <= 0 = |lookat - lookfrom| of the current camera"""
    _fields_ = [("aperture_radius", C.c_double), ("focus_distance", C.c_double), ("flags", C.c_int32), ("reserved", C.c_int32)]


LENS_PROTOTYPES = {
    "take_hip_scene_set_lens": [C.c_void_p, C.POINTER(TakeLens)],
    "take_hip_scene_get_lens": [C.c_void_p, C.POINTER(TakeLens)],
    "take_hip_scene_focus_distance_at": [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_double)],
}


# motion blur (include/take_hip.h)
class TakeShutter(C.Structure):
    """take_hip_render_shutter*: scene time 0 = the marked frame, 1 = the current one; slices <= 0 = min(spp, 16)"""
    _fields_ = [("open", C.c_double), ("close", C.c_double), ("slices", C.c_int32), ("flags", C.c_int32)]


SHUTTER_PROTOTYPES = {
    "take_hip_shutter_plan": [C.c_int32, C.POINTER(TakeShutter), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double)],
    "take_hip_shutter_pose": [C.c_void_p, C.c_double, C.POINTER(TakeCamera), C.c_void_p],
    "take_hip_render_shutter_device": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeShutter), C.c_void_p, C.c_void_p],
    "take_hip_render_shutter": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeShutter), C.c_void_p],
}


class TakeMeshMotion(C.Structure):
    """take_hip_render_shutter_meshes*: the vertex arrays of one mesh at the marked (0) and at the current frame (1), in
    host memory, or all in device memory under TAKE_MESH_DEVICE_ARRAYS; normals: both or neither"""
    _fields_ = [("mesh", C.c_int32), ("flags", C.c_int32), ("positions0", C.c_void_p), ("positions1", C.c_void_p),
                ("normals0", C.c_void_p), ("normals1", C.c_void_p)]


SHUTTER_MESHES_PROTOTYPES = {
    "take_hip_shutter_vertices": [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.POINTER(C.c_int32)],
    "take_hip_shutter_vertices_device": [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p],
    "take_hip_render_shutter_meshes": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeShutter), C.POINTER(TakeMeshMotion), C.c_int32, C.c_void_p],
    "take_hip_render_shutter_meshes_device": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeShutter), C.POINTER(TakeMeshMotion), C.c_int32, C.c_void_p,
                                              C.c_void_p],
}


# the display transform (include/take_hip.h)
TAKE_LUMINANCE_BINS, TAKE_LUMINANCE_SLOTS = 384, 386  # the bins, then [384] non-positive, [385] non-finite
TAKE_TONEMAP_LINEAR, TAKE_TONEMAP_REINHARD, TAKE_TONEMAP_ACES = 0, 1, 2
TAKE_TRANSFER_SRGB, TAKE_TRANSFER_LINEAR = 0, 1
TAKE_DISPLAY_RGBA, TAKE_DISPLAY_REAL = 0, 1
TONEMAP_OPS = {"linear": TAKE_TONEMAP_LINEAR, "reinhard": TAKE_TONEMAP_REINHARD, "aces": TAKE_TONEMAP_ACES}
TRANSFERS = {"srgb": TAKE_TRANSFER_SRGB, "linear": TAKE_TRANSFER_LINEAR}
DISPLAY_FORMATS = {"rgba": TAKE_DISPLAY_RGBA, "real": TAKE_DISPLAY_REAL}


class TakeExposureOpts(C.Structure):
    """take_hip_auto_exposure: a field <= 0 (low_fraction: < 0) takes its default (DISPLAY_DEFAULTS)"""
    _fields_ = [("key", C.c_double), ("low_fraction", C.c_double), ("high_fraction", C.c_double), ("min_exposure", C.c_double),
                ("max_exposure", C.c_double), ("prev_exposure", C.c_double), ("rate", C.c_double)]


class TakeTonemapOpts(C.Structure):
    """take_hip_tonemap*: exposure <= 0 = automatic (with auto_opts), white <= 0 = 4.0"""
    _fields_ = [("exposure", C.c_double), ("white", C.c_double), ("op", C.c_int32), ("transfer", C.c_int32), ("format", C.c_int32),
                ("reserved", C.c_int32), ("auto_opts", TakeExposureOpts)]


DISPLAY_DEFAULTS = {"key": 0.18, "low_fraction": 0.05, "high_fraction": 0.95, "min_exposure": 2.0 ** -16, "max_exposure": 2.0 ** 16, "rate": 1.0,
                    "white": 4.0}


def exposure_opts(key=0.0, low_fraction=-1.0, high_fraction=0.0, min_exposure=0.0, max_exposure=0.0, prev_exposure=0.0, rate=0.0):
    """-> TakeExposureOpts; what is left out takes the library's default (prev_exposure: none, no adaptation)"""
    return TakeExposureOpts(float(key), float(low_fraction), float(high_fraction), float(min_exposure), float(max_exposure),
                            float(prev_exposure or 0.0), float(rate))


def tonemap_opts(exposure=None, op="aces", transfer="srgb", format="rgba", white=0.0, **auto):
    """-> TakeTonemapOpts; exposure None (or <= 0) = automatic, with the keywords of exposure_opts in `auto`; op,
    transfer and format by name (TONEMAP_OPS, TRANSFERS, DISPLAY_FORMATS) or by their TAKE_* value"""
    def pick(table, what, v):
        if isinstance(v, str):
            if v not in table:
                raise ValueError(f"unknown {what} {v!r}: one of {tuple(table)}")
            return table[v]
        return int(v)

    return TakeTonemapOpts(float(exposure or 0.0), float(white), pick(TONEMAP_OPS, "tone operator", op), pick(TRANSFERS, "transfer", transfer),
                           pick(DISPLAY_FORMATS, "format", format), 0, exposure_opts(**auto))


# name -> argument types
DISPLAY_PROTOTYPES = {
    "take_hip_luminance_histogram_device": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_void_p],
    "take_hip_luminance_histogram": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)],
    "take_hip_auto_exposure": [C.POINTER(C.c_int64), C.POINTER(TakeExposureOpts), C.POINTER(C.c_double)],
    "take_hip_tonemap_device": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(TakeTonemapOpts), C.c_void_p, C.POINTER(C.c_double), C.c_void_p],
    "take_hip_tonemap": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(TakeTonemapOpts), C.c_void_p, C.POINTER(C.c_double)],
}


# bloom for the display transform, and the image workspace (include/take_hip.h)
TAKE_BLOOM_MAX_LEVELS = 8


class TakeBloomOpts(C.Structure):
    """take_hip_bloom_layer*, take_hip_tonemap_bloom*: a field < 0 (levels: <= 0) takes its default (BLOOM_DEFAULTS; levels: all)"""
    _fields_ = [("threshold", C.c_double), ("knee", C.c_double), ("intensity", C.c_double), ("levels", C.c_int32), ("reserved", C.c_int32)]


BLOOM_DEFAULTS = {"threshold": 1.0, "knee": 0.5, "intensity": 0.25}


def bloom_opts(threshold=-1.0, knee=-1.0, intensity=-1.0, levels=0):
    """-> TakeBloomOpts; what is left out takes the library's default"""
    return TakeBloomOpts(float(threshold), float(knee), float(intensity), int(levels), 0)


# name -> argument types
BLOOM_PROTOTYPES = {
    "take_hip_image_workspace_create": [C.POINTER(C.c_void_p)],
    "take_hip_image_workspace_destroy": [C.c_void_p],
    "take_hip_bloom_layer_device": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.POINTER(TakeBloomOpts), C.c_void_p, C.c_void_p, C.c_void_p],
    "take_hip_bloom_layer": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.POINTER(TakeBloomOpts), C.c_void_p],
    "take_hip_tonemap_bloom_device": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(TakeTonemapOpts), C.POINTER(TakeBloomOpts), C.c_void_p,
                                      C.POINTER(C.c_double), C.c_void_p, C.c_void_p],
    "take_hip_tonemap_bloom": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(TakeTonemapOpts), C.POINTER(TakeBloomOpts), C.c_void_p,
                               C.POINTER(C.c_double)],
}


# TakeRenderOpts.integrator: the reference's integrators (src/integrator/path_tracing.h:5, :114, :161, :274)
INTEGRATOR_PATH_MIS, INTEGRATOR_RAW, INTEGRATOR_ONE_SAMPLE_MIS, INTEGRATOR_ONE_SAMPLE_MIS_POWER = 0, 1, 2, 3


class TakeRayF(C.Structure):
    _fields_ = [("org", c_float3), ("tmin", C.c_float), ("dir", c_float3), ("tmax", C.c_float)]


class TakeRayD(C.Structure):
    _fields_ = [("org", c_double3), ("tmin", C.c_double), ("dir", c_double3), ("tmax", C.c_double)]


# path tracing of caller-supplied rays, and the scene's own camera rays (include/take_hip.h)
TAKE_RAYS_NORMALIZE = 1  # normalise every direction on the device before use


class TakeRayBatch(C.Structure):
    """take_hip_render_rays*: ray_sets * n ray records (host or device memory), n = output texels; ray_sets 1 or spp"""
    _fields_ = [("rays", C.c_void_p), ("n", C.c_int64), ("ray_sets", C.c_int32), ("first_sample", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


# name -> argument types
RAYS_PROTOTYPES = {
    "take_hip_render_rays_device": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeRayBatch), C.c_void_p, C.c_void_p],
    "take_hip_render_rays": [C.c_void_p, C.POINTER(TakeRenderOpts), C.POINTER(TakeRayBatch), C.c_void_p],
    "take_hip_camera_rays_device": [C.c_void_p, C.POINTER(TakeRenderOpts), C.c_int32, C.c_void_p, C.c_void_p],
    "take_hip_camera_rays": [C.c_void_p, C.POINTER(TakeRenderOpts), C.c_int32, C.c_void_p],
}


class TakeHitF(C.Structure):
    _fields_ = [("shape_id", C.c_int32), ("t", C.c_float), ("u", C.c_float), ("v", C.c_float)]


class TakeHitD(C.Structure):
    _fields_ = [("shape_id", C.c_int32), ("reserved", C.c_int32), ("t", C.c_double), ("u", C.c_double),
                ("v", C.c_double)]


class TakeCounters(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("rays_closest", C.c_uint64), ("rays_shadow", C.c_uint64),
                ("node_visits", C.c_uint64), ("prim_tests", C.c_uint64), ("bounces", C.c_uint64),
                ("ms_trace_closest", C.c_double), ("ms_trace_shadow", C.c_double), ("ms_shade", C.c_double),
                ("ms_other", C.c_double), ("ms_total", C.c_double),
                ("launches_trace_closest", C.c_uint64), ("launches_trace_shadow", C.c_uint64),
                ("node_bytes", C.c_uint64), ("prim_bytes", C.c_uint64), ("leaf_visits", C.c_uint64),
                ("wave_node_steps", C.c_uint64), ("wave_leaf_steps", C.c_uint64),
                ("rays_closest_f32", C.c_uint64), ("ms_trace_closest_f32", C.c_double), ("launches_trace_closest_f32", C.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


# the library itself, scenes, renders, traces, scene groups and EXR egress (include/take_hip.h): name -> argument types
SCENE_PROTOTYPES = {
    "take_hip_last_error": [],
    "take_hip_abi_version": [],
    "take_hip_device_count": [],
    "take_hip_scene_create": [C.POINTER(TakeSceneDesc), C.POINTER(TakeBuildOpts), C.POINTER(C.c_void_p)],
    "take_hip_scene_destroy": [C.c_void_p],
    "take_hip_render": [C.c_void_p, C.POINTER(TakeRenderOpts), C.c_void_p],
    "take_hip_render_device": [C.c_void_p, C.POINTER(TakeRenderOpts), C.c_void_p, C.c_void_p],
    "take_hip_render_accumulate": [C.c_void_p, C.POINTER(TakeRenderOpts), C.c_int32, C.c_void_p, C.c_void_p],
    "take_hip_accumulated_samples": [C.c_void_p],
    "take_hip_render_rows": [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32)],
    "take_hip_trace_closest": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "take_hip_trace_any": [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)],
    "take_hip_trace_closest_device": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p],
    "take_hip_get_counters": [C.c_void_p, C.POINTER(TakeCounters)],
    "take_hip_set_instrumentation": [C.c_void_p, C.c_int32],
    "take_hip_scene_stats": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)],
    "take_hip_scene_build_info": [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
}
GROUP_PROTOTYPES = {
    "take_hip_group_create": [C.POINTER(TakeSceneDesc), C.POINTER(TakeBuildOpts), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_void_p)],
    "take_hip_group_destroy": [C.c_void_p],
    "take_hip_group_render": [C.c_void_p, C.POINTER(TakeRenderOpts), C.c_void_p],
    "take_hip_group_render_device": [C.c_void_p, C.POINTER(TakeRenderOpts), C.c_void_p],
    "take_hip_group_size": [C.c_void_p],
    "take_hip_group_get_counters": [C.c_void_p, C.c_int32, C.POINTER(TakeCounters)],
}
EXR_PROTOTYPES = {
    "take_hip_pack_exr_scanlines": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p],
    "take_hip_render_exr_scanlines": [C.c_void_p, C.POINTER(TakeRenderOpts), C.c_void_p],
}
# the test hooks on the shading functions and on a scene's environment map
DEBUG_PROTOTYPES = {
    "take_hip_debug_table": [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32],
    "take_hip_debug_env": [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p],
}


class TakeDebugTreeInfo(C.Structure):
    _fields_ = [("node_format", C.c_int32), ("node_width", C.c_int32), ("two_level", C.c_int32), ("root_child", C.c_int32),
                ("real_bytes", C.c_int32), ("node_bytes", C.c_int32), ("prim_bytes", C.c_int32), ("inst_bytes", C.c_int32),
                ("n_nodes", C.c_int64), ("n_prims", C.c_int64), ("n_instances", C.c_int64),
                ("grid_lo", c_float3), ("grid_step", c_float3)]


# the test hook that reads a resident tree back (include/take_hip.h: take_hip_debug_tree)
DEBUG_TREE_PROTOTYPES = {
    "take_hip_debug_tree_info": [C.c_void_p, C.c_int32, C.POINTER(TakeDebugTreeInfo)],
    "take_hip_debug_tree": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
}
NODE_FORMAT_WIDE, NODE_FORMAT_Q4, NODE_FORMAT_Q8 = 0, 1, 2


# a new environment map for a resident scene, and the test hook that reads a side's map back (include/take_hip.h)
class TakeEnvImage(C.Structure):
    """take_hip_scene_set_envmap*: height * width * 3 texels, row 0 = zenith; real: TAKE_PRECISION_F32 float texels,
    TAKE_PRECISION_F64 double texels; flags: 0, or TAKE_MESH_DEVICE_ARRAYS = data is device memory"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("data", C.c_void_p), ("real", C.c_int32), ("flags", C.c_int32)]


class TakeDebugEnvTablesInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_guide_m", C.c_int32), ("n_guide_c", C.c_int32),
                ("real_bytes", C.c_int32), ("n_images", C.c_int32), ("texel0", C.c_int64), ("scale", c_double3), ("intensity", c_double3)]


IMAGE_INFO_DTYPE = [("width", "<i4"), ("height", "<i4"), ("offset", "<i8")]  # ImageInfo, take_amd/csrc/tk_scene.h
# name -> argument types
ENVMAP_PROTOTYPES = {
    "take_hip_scene_set_envmap": [C.c_void_p, C.POINTER(TakeEnvImage), C.POINTER(C.c_double)],
    "take_hip_scene_set_envmap_device": [C.c_void_p, C.POINTER(TakeEnvImage), C.POINTER(C.c_double), C.c_void_p],
    "take_hip_debug_env_tables_info": [C.c_void_p, C.c_int32, C.POINTER(TakeDebugEnvTablesInfo)],
    "take_hip_debug_env_tables": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
}


# new materials and light intensities for a resident scene, and the test hook that reads a side's shading tables back
# (include/take_hip.h)
class TakeDebugShadingTablesInfo(C.Structure):
    _fields_ = [("n_materials", C.c_int32), ("n_lights", C.c_int32), ("n_instances", C.c_int64), ("real_bytes", C.c_int32),
                ("material_bytes", C.c_int32), ("light_bytes", C.c_int32), ("inst_shade_bytes", C.c_int32), ("n_pmf", C.c_int32), ("n_cdf", C.c_int32),
                ("tag_mask", C.c_uint32), ("n_material_tags", C.c_int32), ("single_tag", C.c_int32), ("reserved", C.c_int32)]


SHADING_UPDATE_PROTOTYPES = {
    "take_hip_scene_set_materials": [C.c_void_p, C.POINTER(TakeMaterial), C.c_int32, C.c_int32],
    "take_hip_scene_set_light_intensities": [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.c_int32],
    "take_hip_scene_set_light_intensities_device": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p],
    "take_hip_debug_shading_tables_info": [C.c_void_p, C.c_int32, C.POINTER(TakeDebugShadingTablesInfo)],
    "take_hip_debug_shading_tables": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
}


def fill_material(c, m):
    """the TakeMaterial `c` from a take_amd.scene.Material: what SceneData.to_desc and Scene.set_materials both use"""
    c.tag = m.tag
    c.reflectance.kind, c.reflectance.image_id = m.tex_kind, m.tex_image
    c.reflectance.value = c_double3(*m.color)
    c.reflectance.uscale, c.reflectance.vscale, c.reflectance.uoffset, c.reflectance.voffset = m.uvxf
    c.param = (C.c_double * 12)(*(tuple(m.param) + (0.0,) * (12 - len(m.param))))


def shading_table_dtypes(real_bytes):
    """numpy dtypes of the arrays take_hip_debug_shading_tables fills (the layouts of take_amd/csrc/tk_scene.h:
    MaterialRec<Real>, LightRec<Real>, InstShade<Real>) -> (material, light, inst_shade)"""
    import numpy as np

    real, rb = ("<f4", 4) if real_bytes == 4 else ("<f8", 8)
    material = np.dtype({"names": ["tag", "tex_kind", "tex_image", "pad", "color", "uvxf", "p0", "p1", "p"],
                         "formats": ["<i4"] * 4 + [(real, 3), (real, 4), real, real, (real, MATERIAL_PARAMS)],
                         "offsets": [0, 4, 8, 12, 16, 16 + 3 * rb, 16 + 7 * rb, 16 + 8 * rb, 16 + 9 * rb], "itemsize": 16 + (9 + MATERIAL_PARAMS) * rb})
    light = np.dtype({"names": ["kind", "shape_id", "is_sphere", "pad", "intensity", "v", "n"], "formats": ["<i4"] * 4 + [(real, 3), (real, 9), (real, 9)],
                      "offsets": [0, 4, 8, 12, 16, 16 + 3 * rb, 16 + 12 * rb], "itemsize": 16 + 21 * rb})
    inst = np.dtype({"names": ["fwd", "material", "tag", "shape_base", "pad"], "formats": [(real, 9)] + ["<i4"] * 4,
                     "offsets": [0, 9 * rb, 9 * rb + 4, 9 * rb + 8, 9 * rb + 12], "itemsize": 64 if rb == 4 else 96})
    return material, light, inst


def debug_tree_dtypes(info):
    """numpy dtypes of the arrays take_hip_debug_tree fills, from its info (the layouts of take_amd/csrc/tk_scene.h:
    NodeW<Real, 4> / QNodeW<W>, PrimRec<Real>, InstTrace<Real>) -> (node, prim, inst)"""
    import numpy as np

    real = "<f4" if info.real_bytes == 4 else "<f8"
    rb, w = info.real_bytes, info.node_width
    if info.node_format == NODE_FORMAT_WIDE:
        slot = np.dtype({"names": ["bmin", "bmax", "child", "pad"], "formats": [(real, 3), (real, 3), "<i4", "<i4"],
                         "offsets": [0, 3 * rb, 6 * rb, 6 * rb + 4], "itemsize": 32 if rb == 4 else 64})
    else:
        slot = np.dtype([("q", "<u4", 3), ("child", "<i4")])
    node = np.dtype([("c", slot, w)])
    prim = np.dtype({"names": ["a", "shape_id", "meta", "material", "area_light", "nidx", "mesh"],
                     "formats": [(real, 9)] + ["<i4"] * 6, "offsets": [0] + [9 * rb + 4 * k for k in range(6)],
                     "itemsize": 64 if rb == 4 else 96})
    inst = np.dtype({"names": ["inv", "grid_lo", "grid_step", "root_child"], "formats": [(real, 12), ("<f4", 3), ("<f4", 3), "<i4"],
                     "offsets": [0, 12 * rb, 12 * rb + 12, 12 * rb + 24], "itemsize": 80 if rb == 4 else 128})
    assert (node.itemsize, prim.itemsize, inst.itemsize) == (info.node_bytes, info.prim_bytes, info.inst_bytes), "layout of the tree hook changed"
    return node, prim, inst


def debug_tree_result(info, nodes, prims, inst):
    """what Scene.debug_tree and the tests' host twin return: the info as plain values and the three structured arrays"""
    return {"node_format": int(info.node_format), "node_width": int(info.node_width), "two_level": bool(info.two_level),
            "root_child": int(info.root_child), "real_bytes": int(info.real_bytes), "n_nodes": int(info.n_nodes),
            "n_prims": int(info.n_prims), "n_instances": int(info.n_instances), "grid_lo": [float(x) for x in info.grid_lo],
            "grid_step": [float(x) for x in info.grid_step], "nodes": nodes, "prims": prims, "inst_trace": inst}


def _one_table(tables):
    """the union of the *_PROTOTYPES dicts; a name in two of them is a mistake"""
    out = {}
    for table in tables:
        twice = sorted(set(out) & set(table))
        if twice:
            raise RuntimeError(f"{twice[0]} has a prototype in two tables")
        out.update(table)
    return out


# every function include/take_hip.h declares: name -> argument types.  A new entry point goes into the *_PROTOTYPES dict
# beside its structs (or a new dict of that name) and nowhere else; tests/test_capi_cpu.py holds the table against the header
PROTOTYPES = _one_table([v for k, v in sorted(globals().items()) if k.endswith("_PROTOTYPES")])
# the functions that do not return int
RESTYPES = {"take_hip_last_error": C.c_char_p, "take_hip_accumulated_samples": C.c_int64, "take_hip_image_workspace_destroy": None}
