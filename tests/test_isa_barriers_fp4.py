"""tests/test_isa_barriers.py's pin for the fp4 instance of the symmetric Gram
kernel (gram_fp4sym_kernel, csrc/gram_sym.hip): its LDS row accumulator takes
no-return ds_add_u64 from every wave and is flushed by others, so every
s_barrier must sit behind an lgkmcnt(0) wait with no LDS instruction between
(no GPU needed).  The kernel must also be the scaled fp4 MFMA's: the 16x16x128
form with e2m1 on both sides, and no other MFMA in it."""
from test_isa_barriers import _check, _disassemble, _functions


def test_every_fp4_gram_barrier_waits_for_lds():
    funcs = _functions(_disassemble())
    grams = {k: v for k, v in funcs.items() if "gram_fp4sym_kernel" in k}
    assert len(grams) == 1, sorted(grams)
    for name, body in grams.items():
        n, bad = _check(body)
        assert n > 0, name
        assert not bad, (name, bad[:3])
        mfma = [i for i in body if i.startswith("v_mfma")]
        assert len(mfma) == 512, len(mfma)  # 16 column tiles x 2 k-steps x 16 row tiles
        assert all(i.startswith("v_mfma_scale_f32_16x16x128_f8f6f4") for i in mfma)
        assert all("cbsz:4" in i and "blgp:4" in i for i in mfma), mfma[:2]
