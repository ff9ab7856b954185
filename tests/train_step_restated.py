"""The map assembly of the registration training step (reference pipeline/modules/model_pipeline.py:40-104 with
_get_accurate_RT) as plain torch, in the dtype of its inputs: what ops.map_poses / ops.map_assemble compute, with torch's own
inverse and matmul.  tests/test_train_step_host.py pins it to the reference's recorded run; the GPU tests take gradients
through it.  Not a copy of the reference: no frame loop, no dictionary, the host's lookup result (icp, has_icp) is an input."""
import torch


def poses(R, T, calib, icp, has_icp, S, S1):
    """R (F,3,3), T (F,3,1), calib (F,4,4), icp (F+B,16), has_icp (F+B,) -> rel (F,12), gt (B,12), rows [R | T]"""
    F = R.shape[0]
    B = F // S
    dev = R.device
    frame, maps = torch.arange(F, device=dev), torch.arange(B, device=dev)
    first = (frame // S) * S + torch.where(frame % S < S1, 0, S1)
    src = torch.cat([frame, maps * S])
    dst = torch.cat([first, maps * S + S1])
    with_icp = (calib[dst] @ icp.reshape(-1, 4, 4).to(R.dtype) @ torch.linalg.inv(calib[src]))[:, :3]
    Rc = R[dst].transpose(1, 2)
    without = torch.cat([Rc @ R[src], Rc @ (T[src] - T[dst])], dim=2)
    out = torch.where(has_icp.to(dev).bool().reshape(-1, 1, 1), with_icp, without)
    out[:F][frame == first] = torch.eye(3, 4, dtype=R.dtype, device=dev)
    return out[:F].reshape(F, 12), out[F:].reshape(B, 12)


def assemble(coor, fea, mask, rel, gt, S, S1, coor_scale):
    """-> src_desc, dst_desc, src_mask, dst_mask, src_global, dst_global (see ops.map_assemble)"""
    F, C, N = fea.shape
    B = F // S
    rel = rel.reshape(F, 3, 4)
    p = coor * coor_scale
    moved = rel[:, :, :3] @ p + rel[:, :, 3:]
    place = torch.arange(F, device=fea.device) % S
    is_first = (place == 0) | (place == S1)
    xyz = torch.where(is_first.reshape(F, 1, 1), p, moved)
    desc = torch.cat([fea, xyz], dim=1).reshape(B, S, C + 3, N)
    m = mask.reshape(B, S, N)
    to_map = lambda t: t.transpose(1, 2).reshape(B, C + 3, -1)   # noqa: E731
    src_desc, dst_desc = to_map(desc[:, :S1]), to_map(desc[:, S1:])
    gt = gt.reshape(B, 3, 4)
    src_global = gt[:, :, :3] @ src_desc[:, C:].detach() + gt[:, :, 3:]
    return (src_desc, dst_desc, m[:, :S1].reshape(B, -1), m[:, S1:].reshape(B, -1), src_global, dst_desc[:, C:].detach().clone())
