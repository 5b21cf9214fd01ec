"""Growing the deformation graph from the fused volume: new nodes where the sampled model leaves the graph's coverage.

DynamicFusion extends its graph after every integrate: surface points that no node supports are subsampled at the node
spacing, their transforms are blended from the neighbours and the regularisation graph is extended. The reference's
route is EDGraph.update behind WarpField.find_unreachable_nodes (embedded_deformation_graph.py:496-609, warpfield.py:
462-485): marching cubes, a host greedy loop, new geodesic edges and a host ARAP solve; its drivers keep it commented
out. NodeGrower works on the rows WarpField.surface_points(sync=False) writes — every point brings its voxel's anchors
and weights — in one stream-ordered call (torch.ops.ofx.grow_nodes -> ofx_grow_nodes). The contract is in include/ofx.h
and restated by tests/grow_ref.py.
"""
import torch

from . import _lib, ops  # noqa: F401  (ops registers torch.ops.ofx.*)
from ._lib import byref, call

MAX_POINTS = 65536   # model rows a handle can take (ofx_grow_create)
MAX_NEW = 4096       # nodes one call can add: the selected positions live in LDS


class NodeGrower:
    """Owns an ofx_grow handle (candidate flags, their ranks and the candidate / selected row lists for up to
    max_points model rows and max_new new nodes a call)."""

    def __init__(self, max_points, max_new, device=None):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.max_points, self.max_new = int(max_points), int(max_new)
        self._h = _lib.c_void_p()
        with torch.cuda.device(self.device):
            call("ofx_grow_create", self.max_points, self.max_new, byref(self._h))
        self._state = torch.zeros(1, dtype=torch.int32, device=self.device)   # ofx::grow_nodes ordering token

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.lib.ofx_grow_destroy(h)
            except Exception:
                pass
        self._h = None

    def grow(self, points, anchors, weights, valid, nodes, n_nodes, rotations, translations, edges, edge_weights,
             node_coverage, min_dist=None, spacing=None, max_new=None, count=None):
        """Append up to max_new nodes to the caller's device arrays, which hold n_nodes rows and room for max_new more
        (nodes (.,3), rotations (.,3,3), translations (.,3), edges i32 (.,K_e), edge_weights (.,K_e)), from the padded
        model rows (points, anchors i32, weights, valid u8). min_dist defaults to 2·node_coverage (the reference's
        find_unreachable_nodes), spacing to node_coverage. -> count, device int32 (3,) = [candidates, selected, capped];
        enqueued on torch's current stream without a host read."""
        cov = float(node_coverage)
        max_new = self.max_new if max_new is None else int(max_new)
        if count is None:
            count = torch.empty(3, dtype=torch.int32, device=self.device)
        torch.ops.ofx.grow_nodes(self._state, self._h.value, points, anchors, weights, valid, nodes, int(n_nodes),
                                 rotations, translations, edges, edge_weights, cov,
                                 2.0 * cov if min_dist is None else float(min_dist),
                                 cov if spacing is None else float(spacing), max_new, count)
        return count
