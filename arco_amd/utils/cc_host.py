"""Connected components BY VALUE on the host (scipy): the host twins of cc_gpu.largest_cc_by_value and cc_gpu.largest_per_class.

test_util.getLargestCC takes every non-zero label as one foreground; skimage.measure.label, which the reference's getLargestCC calls
(test_util.py:11-15), joins only neighbours of the SAME value.  The two agree on binary maps and differ from three classes on.
  getLargestCC_by_value(segmentation)   the reference's meaning: the largest component of any single value, a bool array
  keep_largest_per_class(segmentation)  the label map with all but each value's largest component zeroed - the usual post-processing
                                        of multi-class predictions
scipy.ndimage.label once per distinct non-zero value, full connectivity.  Of several components of one size the one whose first voxel
comes first in memory wins, which is `argmax(bincount(labels.flat)[1:])` on a raster-order numbering.  Not pinned to skimage itself,
which is not a dependency."""
import numpy as np


def _largest_by_value(seg):
    """[(value, its largest component as a bool array, that component's first flat index, its voxel count)] over the distinct non-zero
    values of `seg` in ascending order."""
    from scipy.ndimage import generate_binary_structure, label
    structure = generate_binary_structure(seg.ndim, seg.ndim)
    out = []
    for value in np.unique(seg):
        if value == 0:
            continue
        labels, _ = label(seg == value, structure=structure)
        counts = np.bincount(labels.flat)[1:]
        mask = labels == np.argmax(counts) + 1
        out.append((value, mask, int(np.argmax(mask)), int(counts.max())))
    return out


def getLargestCC_by_value(segmentation):
    """getLargestCC as the reference computes it: the largest component of equal values (ties: the first in memory).  Equal to
    test_util.getLargestCC on a binary map.  AssertionError without foreground, as that function."""
    found = _largest_by_value(np.asarray(segmentation))
    assert len(found) != 0               # assume at least 1 CC
    size = max(n for _, _, _, n in found)
    _, mask = min(((first, mask) for _, mask, first, n in found if n == size), key=lambda t: t[0])
    return mask


def keep_largest_per_class(segmentation):
    """The label map with all but the largest component (full connectivity) of every non-zero value zeroed.  Ties as above."""
    seg = np.asarray(segmentation)
    out = np.zeros_like(seg)
    for value, mask, _, _ in _largest_by_value(seg):
        out[mask] = value
    return out
