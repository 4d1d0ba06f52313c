"""`PG_OP`-shaped module: the 15 functions DODA's lib/pointgroup_ops/functions/pointgroup_ops.py
calls on its pybind extension (reference lib/pointgroup_ops/src/pointgroup_ops_api.cpp:6-26),
with the same positional signatures, backed by libdoda_hip.so (include/doda_hip.h for the voxel,
ball-query and kNN entry points, include/doda_pgops.h for clustering, the segment pools and the
proposal IoU).  bfs_cluster takes CPU tensors (the reference's route: a sequential BFS on the host)
or device tensors (connected components on the device: the same clusters in the same order on a
symmetric neighbour graph, points inside a cluster ascending); the other seven need device tensors."""
from . import ops as _ops


def voxelize_idx(coords, output_coords, input_map, output_map, batch_size, mode):
    """pointgroup_ops.cpp:14-17 -> voxelize.cpp:10-31.  Resizes output_coords / output_map like
    the reference (`resize_` + fill).  CPU tensors run the fork-safe host path (DataLoader
    workers); device tensors run the HIP path."""
    if coords.is_cuda:
        oc, im, om = _ops.voxelize_idx_device(coords, batch_size, mode)
    else:
        oc, im, om = _ops.voxelize_idx_host(coords, batch_size, mode)
    output_coords.resize_(oc.shape).copy_(oc)
    output_map.resize_(om.shape).copy_(om)
    input_map.copy_(im)


def voxelize_fp(feats, output_feats, output_map, mode, n_active, max_active, n_plane):
    _ops.voxelize_fp(feats, output_feats, output_map, mode, n_active, max_active, n_plane)


def voxelize_bp(d_output_feats, d_feats, output_map, mode, n_active, max_active, n_plane):
    _ops.voxelize_bp(d_output_feats, d_feats, output_map, mode, n_active, max_active, n_plane)


def point_recover_fp(feats, output_feats, idx_map, n_active, max_active, n_plane):
    _ops.point_recover_fp(feats, output_feats, idx_map, n_active, max_active, n_plane)


def point_recover_bp(d_output_feats, d_feats, idx_map, n_active, max_active, n_plane):
    _ops.point_recover_bp(d_output_feats, d_feats, idx_map, n_active, max_active, n_plane)


def ballquery_batch_p(xyz, batch_idxs, batch_offsets, idx, start_len, n, mean_active, radius):
    return _ops.ballquery_batch_p(xyz, batch_idxs, batch_offsets, idx, start_len, n, mean_active,
                                  radius)


def knn_batch(xyz, query_xyz, batch_idxs, query_batch_offsets, idx, n, m, k):
    _ops.knn_batch(xyz, query_xyz, batch_idxs, query_batch_offsets, idx, n, m, k)


def bfs_cluster(semantic_label, ball_query_idxs, start_len, cluster_idxs, cluster_offsets, n, threshold):
    """pointgroup_ops_api.cpp:19 -> bfs_cluster.cpp:93-112.  Resizes and fills cluster_idxs [sumNPoint, 2] and cluster_offsets
    [nCluster + 1] like the reference (`resize_` + fill).  CPU tensors run the reference's sequential BFS on the host; device
    tensors run the union-find components on the device."""
    if int(n) != start_len.shape[0]:
        raise RuntimeError("bfs_cluster: N must be start_len's row count")
    route = _ops.pg_cluster if semantic_label.is_cuda else _ops.pg_bfs_cluster_host
    idxs, offsets = route(semantic_label, ball_query_idxs, start_len, threshold)
    cluster_idxs.resize_(idxs.shape).copy_(idxs)
    cluster_offsets.resize_(offsets.shape).copy_(offsets)


def roipool_fp(feats, proposals_offset, output_feats, output_maxidx, n_proposal, n_plane):
    _ops.roipool_fp(feats, proposals_offset, output_feats, output_maxidx, n_proposal, n_plane)


def roipool_bp(d_feats, proposals_offset, output_maxidx, d_output_feats, n_proposal, n_plane):
    _ops.roipool_bp(d_feats, proposals_offset, output_maxidx, d_output_feats, n_proposal, n_plane)


def get_iou(proposals_idx, proposals_offset, instance_labels, instance_pointnum, proposals_iou, n_instance, n_proposal):
    _ops.get_iou(proposals_idx, proposals_offset, instance_labels, instance_pointnum, proposals_iou, n_instance, n_proposal)


def sec_mean(inp, offsets, out, n_proposal, n_plane):
    _ops.sec_mean(inp, offsets, out, n_proposal, n_plane)


def sec_mean_bp(d_inp, offsets, d_out, n_proposal, n_plane):
    """Note the reference's argument order (sec_mean.cpp:17): the gradient to fill comes first."""
    _ops.sec_mean_bp(d_inp, offsets, d_out, n_proposal, n_plane)


def sec_min(inp, offsets, out, n_proposal, n_plane):
    _ops.sec_min(inp, offsets, out, n_proposal, n_plane)


def sec_max(inp, offsets, out, n_proposal, n_plane):
    _ops.sec_max(inp, offsets, out, n_proposal, n_plane)
