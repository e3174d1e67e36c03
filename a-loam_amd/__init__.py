"""a-loam_amd — what the MI355X A-LOAM hot path needs, nothing else.

csrc/       HIP kernels (gfx950) + the C-ABI host side -> lib/libaloam_mi355x.so (include/aloam_mi355x.h)
host/       the three ROS node shims that keep the aloam_velodyne topic surface and call the C ABI
binding.py  ctypes stub of the C ABI (tests, bench.py); no second implementation
records.py  the header's records (ctypes structures, the numpy dtypes made from them) and enumerators, declared once
synthetic.py  seeded synthetic sweeps (regular and KITTI-shaped rough ones); shard.py  sequence -> rank assignment
atlas.py    map tiles on the host (numpy): what the map spill drains, files, the window-shift model
KITTI-layout input and ground-truth evaluation live in tools/run_kitti.py.
"""
