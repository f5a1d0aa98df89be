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

A frame is one upload, crop -> FPS -> labels on the device, one download.  There is no CPU path.
"""
