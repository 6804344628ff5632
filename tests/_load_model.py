"""numpy model of the canonical build of a dense voxel volume (bm_scene_load_voxels), written from the rules in include/brickmap.h:
a brick per cell that holds a solid voxel, bit x + 8 y + 64 z, host slots 0, 1, 2 ... in ascending local cell index bx + 16 by + 256 bz,
word = slot | loaded | lod << 12 with lod bit (x >= 4) + 2 (y >= 4) + 4 (z >= 4) set iff that octant of the brick holds a solid voxel."""
import numpy as np


def canonical_supercell(volume, sx, sy, sz):
    """(words[4096], bricks[n, 16]) of supercell (sx, sy, sz) of `volume` ([z, y, x], non-zero = solid)"""
    sub = volume[sz * 128:sz * 128 + 128, sy * 128:sy * 128 + 128, sx * 128:sx * 128 + 128] != 0
    cells = sub.reshape(16, 8, 16, 8, 16, 8).transpose(0, 2, 4, 1, 3, 5).reshape(4096, 512)  # [bz, by, bx] -> local cell; [z, y, x] -> bit
    occupied = cells.any(1)
    slots = (np.cumsum(occupied) - 1).astype(np.uint32)
    bricks = np.packbits(cells, axis=1, bitorder="little").view(np.uint32)
    octants = cells.reshape(4096, 2, 4, 2, 4, 2, 4).any(axis=(2, 4, 6)).reshape(4096, 8)  # [qz, qy, qx] -> bit 4 qz + 2 qy + qx
    lod = (octants.astype(np.uint32) << np.arange(8, dtype=np.uint32)).sum(1).astype(np.uint32)
    words = np.where(occupied, slots | np.uint32(0x80000000) | (lod << np.uint32(12)), np.uint32(0)).astype(np.uint32)
    return words, np.ascontiguousarray(bricks[occupied])


def expand_supercell(volume, sx, sy, sz, words, bricks):
    """write the voxels of one supercell (its words and bricks) into `volume`"""
    for cell in np.nonzero(words)[0]:
        bits = np.unpackbits(bricks[words[cell] & 0xFFF].view(np.uint8), bitorder="little").reshape(8, 8, 8)
        x, y, z = sx * 128 + (cell & 15) * 8, sy * 128 + ((cell >> 4) & 15) * 8, sz * 128 + (cell >> 8) * 8
        volume[z:z + 8, y:y + 8, x:x + 8] = bits
