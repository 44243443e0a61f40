"""MI355X-native U-Net segmentation engine (drop-in for the reference's U-Net hot path).

Public surface:
  runners.holdout_runner_unet_infection_segmentation / runners.runner_lung_segmentation
  keras_like.UNetModel   -- compile / fit / evaluate / predict / save_weights / load_weights
  volume.segment_volume / volume.build_dataset / volume.load_volume -- a NIfTI CT volume in, slice batches / a mask volume out (nifti_min reads the file)
  split_lungs / lung_burden (LungSides, LungBurden, LungSplitError) -- volume's left / right lung split and per-lung burden, also reachable from the package itself
  render_planes / project_volume / key_slices (Layer, RenderedSheet) -- volume's pictures of a segmented CT, also reachable from the package itself; png_min writes them
  resample_volume / resample_mask / resample_labels / reorient_volume / change_between (Grid, ResampledVolume, VolumeChange) -- volume's resampling onto another grid,
                            also reachable from the package itself
  extract_surface / lesion_shapes (SurfaceMesh) -- volume's triangle meshes of a mask, a label volume or a scalar volume, also reachable from the package itself;
                            mesh_min writes them as STL / PLY / OBJ
  track_lesions / track_series / label_pairs / match_lesions (LesionTracking, LesionSeries, LesionMatch, PALETTE_CHANGE) -- tracking's per-lesion follow-up: every lesion
                            of a baseline matched to the follow-up's (persistent / merged / split / complex / new / resolved), also reachable from the package itself
  texture_stats / lesion_texture / glcm / run_lengths / quantize_volume / glcm_features / run_features (TextureStats) -- texture's second-order texture of the CT under a
                            mask: grey-level co-occurrence and run-length matrices per lesion or per lung, also reachable from the package itself
  lung_zones / lung_distribution (LungZones, LungDistribution) -- zones' answer to WHERE the infection sits: every lung voxel by side x anatomical zone x depth shell under
                            the lung surface, a severity score per region and the words of a report (bilateral, upper / lower, peripheral / central), also reachable
                            from the package itself
  rank_filter / median_filter / minimum_filter / maximum_filter / percentile_filter / grey_erosion / grey_dilation / grey_opening / grey_closing / gaussian_filter
                            (FilteredVolume, footprint_bits, structure) -- filters' changes to the CT's own voxels: the element of a rank under a footprint of radius
                            <= 2, exact against scipy.ndimage, and the Gaussian low-pass to run before resample_volume coarsens, also reachable from the package itself
  lung_mask / threshold_volume / geodesic_distance / reconstruct / body_mask / find_trachea / grow_airways (LungMask, AirwayGrowth, TracheaSeed, LungMaskError) -- lungs'
                            lung mask from the CT itself: the air inside the body, trachea and main bronchi grown from a seed and removed, the two lungs kept; also
                            reachable from the package itself
  hessian_eigenvalues / vesselness / vessel_mask (Vesselness, VesselMask) -- vessels' tube measure of the CT: the eigenvalues of the scale-normalised Hessian, Frangi's
                            vesselness over a few scales and the vessel mask inside the lungs that segment_volume(vessels=) reports the infection against; also
                            reachable from the package itself
  thin_volume / skeleton_table / skeleton_graph / prune / root_tree / branch_territories / airway_tree / vessel_tree (Skeleton, SkeletonGraph, RootedTree,
                            BranchTerritories, CenterlineTree) -- skeleton's centerlines of the airway and vessel masks: topology-preserving thinning on the device, the
                            branch graph with lengths and calibres, generations from a root and the mask voxels of every branch; also reachable from the package itself
  watershed / watershed_device / depth_cost_device / split_lesions (WatershedResult, SplitLesions, WatershedError) -- watershed's marker-controlled watershed over an
                            integer cost volume (pass height, then labels along the edges that realise it; or the summed cost) and the split of touching lesions
                            into parts grown from the cores of the distance transform; also reachable from the package itself
  engine.HipUNet         -- the HIP backend (libunet_hip.so through the C ABI of include/unet_hip.h)
Importing this package has no side effects and does not need a GPU; constructing the
backend does (there is no CPU fallback).
"""
__all__ = ["runners", "keras_like", "engine", "weights", "data", "volume", "nifti_min", "png_min", "mesh_min", "split_lungs", "lung_burden", "LungSides", "LungBurden", "LungSplitError",
           "render_planes", "project_volume", "key_slices", "Layer", "RenderedSheet", "resample_volume", "resample_mask", "resample_labels", "reorient_volume", "change_between",
           "Grid", "ResampledVolume", "VolumeChange", "extract_surface", "lesion_shapes", "SurfaceMesh", "tracking", "track_lesions", "track_series", "label_pairs", "match_lesions",
           "LesionTracking", "LesionSeries", "LesionMatch", "PALETTE_CHANGE", "texture", "texture_stats", "lesion_texture", "glcm", "run_lengths", "quantize_volume", "glcm_features",
           "run_features", "TextureStats", "zones", "lung_zones", "lung_distribution", "LungZones", "LungDistribution", "filters", "rank_filter", "median_filter", "minimum_filter", "maximum_filter", "percentile_filter",
           "grey_erosion", "grey_dilation", "grey_opening", "grey_closing", "gaussian_filter", "footprint_bits", "structure", "FilteredVolume",
           "lungs", "lung_mask", "threshold_volume", "geodesic_distance", "reconstruct", "body_mask", "find_trachea", "grow_airways", "LungMask", "AirwayGrowth", "TracheaSeed",
           "LungMaskError", "vessels", "hessian_eigenvalues", "vesselness", "vessel_mask", "Vesselness", "VesselMask",
           "skeleton", "thin_volume", "skeleton_table", "skeleton_graph", "prune", "root_tree", "branch_territories", "airway_tree", "vessel_tree", "Skeleton", "SkeletonGraph",
           "RootedTree", "BranchTerritories", "CenterlineTree",
           "watershed", "watershed_device", "depth_cost_device", "split_lesions", "split_lesions_device", "WatershedResult", "SplitLesions", "WatershedError"]
_FROM_VOLUME = ("split_lungs", "lung_burden", "LungSides", "LungBurden", "LungSplitError", "render_planes", "project_volume", "key_slices", "Layer", "RenderedSheet",
                "resample_volume", "resample_mask", "resample_labels", "reorient_volume", "change_between", "Grid", "ResampledVolume", "VolumeChange",
                "extract_surface", "lesion_shapes", "SurfaceMesh")
_FROM_TRACKING = ("track_lesions", "track_series", "label_pairs", "match_lesions", "LesionTracking", "LesionSeries", "LesionMatch", "PALETTE_CHANGE")
_FROM_ZONES = ("lung_zones", "lung_distribution", "LungZones", "LungDistribution")
_FROM_FILTERS = ("rank_filter", "median_filter", "minimum_filter", "maximum_filter", "percentile_filter", "grey_erosion", "grey_dilation", "grey_opening", "grey_closing",
                 "gaussian_filter", "footprint_bits", "structure", "FilteredVolume")
_FROM_LUNGS = ("lung_mask", "threshold_volume", "geodesic_distance", "reconstruct", "body_mask", "find_trachea", "grow_airways", "LungMask", "AirwayGrowth", "TracheaSeed",
               "LungMaskError")
_FROM_VESSELS = ("hessian_eigenvalues", "vesselness", "vessel_mask", "Vesselness", "VesselMask")
_FROM_SKELETON = ("thin_volume", "skeleton_table", "skeleton_graph", "prune", "root_tree", "branch_territories", "airway_tree", "vessel_tree", "Skeleton", "SkeletonGraph",
                  "RootedTree", "BranchTerritories", "CenterlineTree")
_FROM_WATERSHED = ("watershed_device", "depth_cost_device", "split_lesions", "split_lesions_device", "WatershedResult", "SplitLesions", "WatershedError")
_FROM_TEXTURE = ("texture_stats", "lesion_texture", "glcm", "run_lengths", "quantize_volume", "glcm_features", "run_features", "TextureStats")


def __getattr__(name):                                              # resolved on first use: importing the package stays free of side effects
    if name in _FROM_VOLUME:
        import importlib
        return getattr(importlib.import_module(__name__ + ".volume"), name)
    if name in _FROM_TRACKING:
        import importlib
        return getattr(importlib.import_module(__name__ + ".tracking"), name)
    if name in _FROM_TEXTURE:
        import importlib
        return getattr(importlib.import_module(__name__ + ".texture"), name)
    if name in _FROM_ZONES:
        import importlib
        return getattr(importlib.import_module(__name__ + ".zones"), name)
    if name in _FROM_FILTERS:
        import importlib
        return getattr(importlib.import_module(__name__ + ".filters"), name)
    if name in _FROM_LUNGS:
        import importlib
        return getattr(importlib.import_module(__name__ + ".lungs"), name)
    if name in _FROM_VESSELS:
        import importlib
        return getattr(importlib.import_module(__name__ + ".vessels"), name)
    if name in _FROM_SKELETON:
        import importlib
        return getattr(importlib.import_module(__name__ + ".skeleton"), name)
    if name in _FROM_WATERSHED:
        import importlib
        return getattr(importlib.import_module(__name__ + ".watershed"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
