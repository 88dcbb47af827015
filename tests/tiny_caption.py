"""The tiny captioning model of the decode tests (Swin 32 / [2, 2, 2, 2], BERT 256 x 2 layers x 4 heads, 3000 tokens) with the
hash weights of tests/golden/specs_hash.json."""
from conftest import hash_sd


def tiny_caption(M, specs_hash, cd, max_length=8, eos=None):
    cfg = M.MVLBertConfigForImageCaption(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024,
                                         vocab_size=3000)
    cfg.swin.update(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], drop_path_rate=0.2)
    cfg.max_length = max_length
    cfg.eos_token_id = eos
    tok = type("Tok", (), {"mask_token_id": 103, "sep_token_id": 102})()
    model = M.MVLBertForImageCaption(cfg, tokenizer=tok)
    sd = hash_sd(specs_hash["hash_tiny_caption"])
    _, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected
    return M.set_compute_dtype(model.cuda().eval(), cd), sd
