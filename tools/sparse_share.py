"""share of the states the sparse initialisation writes (dev.StatePrepare(sparse_reach=2)): of the 32-voxel groups, which is
the share of the bytes, and of the 1024-voxel chunks it writes anything in; sphere and depth pairs"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from levelsetfusion_python_amd import device as dev
from levelsetfusion_python_amd.synthetic import sphere_pair, depth_pair
for n in (128, 192, 256, 384, 512):
    c, l = sphere_pair(n, 3, "cuda")
    band = float((~((l.abs() == 1) & (c.abs() == 1))).float().mean())
    out = []
    for reach in (1, 2):
        p = dev.StatePrepare(l, c, sparse_reach=reach)
        p.collect()
        out.append((p.written_fraction(), p.needed_fraction()))
    print("sphere pair %d^3: band %.1f %% of the voxels; groups written with reach 1 / 2: %.1f %% / %.1f %% (chunks touched: %.1f %% / %.1f %%)"
          % (n, 100 * band, 100 * out[0][0], 100 * out[1][0], 100 * out[0][1], 100 * out[1][1]))
for n in (256, 512):
    c, l = depth_pair(n, "cuda")
    band = float((~((l.abs() == 1) & (c.abs() == 1))).float().mean())
    p = dev.StatePrepare(l, c, sparse_reach=2)
    p.collect()
    print("depth pair %d^3: band %.1f %% of the voxels; groups written with reach 2: %.1f %% (chunks touched: %.1f %%)"
          % (n, 100 * band, 100 * p.written_fraction(), 100 * p.needed_fraction()))
