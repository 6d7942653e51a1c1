"""TEST INFRASTRUCTURE: the data-gradient chain of the network in double precision, as the yardstick of the gradient
workspace the data-gradient kernels leave (csrc/mlp_bwd.hip, mlp_bwd_h3_kernel.h): the transposed layers, in torch on the
device, on the ReLU decisions of the SAME saved activations the kernels read -- so the comparison holds no gate flip."""
import torch

from scnerf_amd import mlp_layout as ML


def tiled_rows(buf, offset, width, P):
    """row-major [P, width] view of a tile-native section (mlp_layout.untile) of a workspace on the device"""
    Pp = ML.padded_samples(P)
    return buf[offset: offset + width * Pp].view(Pp // 32, width // 32, 4, 2, 32, 4).permute(0, 4, 1, 2, 3, 5).reshape(Pp, width)[:P]


def grad_rows(grads, name, width, P):
    goff, _ = ML.section_offsets(ML.GRAD_SECTIONS, P)
    return tiled_rows(grads, goff[name], width, P)


def fp64_chain(p, save, d_raw, P, pd=3):
    """{section of mlp_layout.GRAD_SECTIONS: fp64 [P, width]}: dZ of the views layer, d feature, dZ of trunk layers 7 .. 0
    from d_raw [P, 4] (rgb logits, sigma), the parameters `p` (name -> tensor) and the activation workspace `save`."""
    lay = ML.layout(pd)
    off, _ = ML.section_offsets(lay.save_sections, P)
    dev = save.device

    def srows(name, width=256):
        return tiled_rows(save, off[name], width, P)
    W = lambda name: p[name].to(dev).double()
    dr = d_raw.double()
    ref = {}
    ref["dzv"] = (dr[:, :3] @ W("rgb_linear.weight")) * (srows("hv", 128) > 0)
    ref["dfeat"] = (ref["dzv"] @ W("views_linears.0.weight"))[:, :256]
    d = (ref["dfeat"] @ W("feature_linear.weight") + dr[:, 3:4] * W("alpha_linear.weight")) * (srows("act7") > 0)
    ref["dz7"] = d
    for l in range(7, 0, -1):
        w_l = W("pts_linears.%d.weight" % l)
        if l == 5:
            w_l = w_l[:, lay.in_pts:]                       # (the skip layer's activation columns)
        d = (d @ w_l) * (srows("act%d" % (l - 1)) > 0)
        ref["dz%d" % (l - 1)] = d
    return ref


def row_errors(grads, ref, name, width, P, keep):
    """largest |difference| of every kept row of section `name` over the row's largest fp64 entry"""
    a = grad_rows(grads, name, width, P).double()
    size = ref[name].abs().max(1)[0].clamp_min(1e-300)
    return ((a - ref[name]).abs().max(1)[0] / size)[keep]
