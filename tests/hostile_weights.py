"""TEST INFRASTRUCTURE: a network the resident arithmetic's scale bound cannot serve (csrc/resident_guard.h).

"hostile" is tests/trained_weights.py's "adversarial" recipe with the cancellation row of pts_linears.3 at 2^18 x the other
rows' 1-norm instead of 2^10: every sample's scale for layer 3's output sits eighteen octaves below where its values would
put it, past the three octaves of head-room the cut has (mlp_h3.h:18-26) -- every sample trips the guard at layer 3."""
import torch

ROW_GAIN = 2.0 ** 18


def weights(seed=0):
    """-> state dict (name -> fp32 CPU tensor) of the standard SCNeRF network (pd = 3)"""
    from scnerf_amd import synthetic as synth
    p = {k: v.clone() for k, v in synth.network_params(seed=seed).items()}
    g = torch.Generator().manual_seed(4242 + seed)
    w1 = p["pts_linears.1.weight"]
    p["pts_linears.1.weight"] = w1 * torch.exp2(torch.randint(-20, 5, w1.shape, generator=g).float())
    w2, b2 = p["pts_linears.2.weight"], p["pts_linears.2.bias"]
    w2[1::2] = w2[0::2]
    b2[1::2] = b2[0::2]
    w3 = p["pts_linears.3.weight"]
    c = float(w3.abs().sum(1).median()) * ROW_GAIN / 256.0
    w3[7, 0::2] = c
    w3[7, 1::2] = -c
    return p
