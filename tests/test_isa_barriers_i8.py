"""tests/test_isa_barriers.py's pin for the int8 instance of the symmetric Gram
kernel (gram_i8sym_kernel, csrc/gram_sym.hip): its LDS row accumulator takes
no-return ds_add_u64 from every wave and is flushed by others, so every
s_barrier must sit behind an lgkmcnt(0) wait with no LDS instruction between
(no GPU needed).  The kernel must also be the int8 MFMA's: no fp16 MFMA in it."""
from test_isa_barriers import _check, _disassemble, _functions


def test_every_i8_gram_barrier_waits_for_lds():
    funcs = _functions(_disassemble())
    grams = {k: v for k, v in funcs.items() if "gram_i8sym_kernel" in k}
    assert len(grams) == 1, sorted(grams)
    for name, body in grams.items():
        n, bad = _check(body)
        assert n > 0, name
        assert not bad, (name, bad[:3])
        assert sum(i.startswith("v_mfma_i32_16x16x64_i8") for i in body) > 0
        assert not any(i.startswith("v_mfma_f32") for i in body)
