"""Data preparation on the device (reference: data_prepare/{kittidet,semantickitti,waymo}/process_*.py): raw scans -> the files
the readers of ogc_amd/datasets.py load.

  scan_ops               crop_camera / crop_front / box_segm — the operators over csrc/scan_prepare.hip
  kitti_io               calibration and label parsers, box rows for box_segm
  process_kittidet       python -m ogc_amd.data_prepare.process_kittidet <data_root>
  process_semantickitti  python -m ogc_amd.data_prepare.process_semantickitti <data_root>
  process_waymo          python -m ogc_amd.data_prepare.process_waymo --data_root R --save_root S --split_file F --cfg_file C
  png16                  read_png / write_png for 8- and 16-bit grey and RGB PNGs (zlib + ogc_png_unfilter)
  process_kittisf        python -m ogc_amd.data_prepare.process_kittisf <data_root>          (scan_ops.kittisf_unproject)
  downsample_kittisf     python -m ogc_amd.data_prepare.downsample_kittisf <data_root> --save_root S [--predflow_path NAME]
  downsample_waymo       python -m ogc_amd.data_prepare.downsample_waymo --data_root R --save_root S --split_file F
  filter_empty           python -m ogc_amd.data_prepare.filter_empty --data_root R --split_file F --out <split>_sup.json   (no device)
  select_mov             python -m ogc_amd.data_prepare.select_mov --data_root S --pose_root R --split_file F --sup_frames J --out_dir D
                         (scan_ops.moving_stats / moving_counts over csrc/moving_stats.hip)
  mesh_ops               surface_candidates / surface_thin / nearest_label and sample_surface_even — the operators over
                         csrc/surface_candidates.hip, surface_thin.hip and nearest_label.hip
  mesh_io                read_obj / write_obj, read_pcd / write_pcd (numpy only)
  sample_pointcloud      python -m ogc_amd.data_prepare.sample_pointcloud <data_root> --save_root S [--keep_background]
  collect_segm           python -m ogc_amd.data_prepare.collect_segm --src_root <OGC-DR root> --dest_root <OGC-DRSV root>
  build_ogcdrsv          python -m ogc_amd.data_prepare.build_ogcdrsv --src_root <OGC-DR root> --dest_root <OGC-DRSV root>
                         (mesh_ops.default_view / depth_render / render_points over csrc/depth_render.hip)
  build_ogcdr            python -m ogc_amd.data_prepare.build_ogcdr <data_root> --split_root <raw_splits> [--keep_background]
                         (mesh_ops.compose_rooms / apply_poses over csrc/room_compose.hip)

A frame is one upload, crop -> FPS -> labels on the device, one download.  There is no CPU path.
"""

_EXPORTS = {"surface_candidates": "mesh_ops", "surface_thin": "mesh_ops", "nearest_label": "mesh_ops", "sample_surface_even": "mesh_ops",
            "default_view": "mesh_ops", "depth_render": "mesh_ops", "render_points": "mesh_ops",
            "compose_rooms": "mesh_ops", "apply_poses": "mesh_ops",
            "read_obj": "mesh_io", "write_obj": "mesh_io", "read_pcd": "mesh_io", "write_pcd": "mesh_io"}
__all__ = sorted(_EXPORTS)


def __getattr__(name):
    # on first use: the drivers above are run as modules and must not find themselves imported already
    if name in _EXPORTS:
        import importlib
        return getattr(importlib.import_module("." + _EXPORTS[name], __name__), name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
