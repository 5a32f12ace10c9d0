"""Text-level generation: Engine.Generate / GenerateQuiet (go/main.go:152-291) = tokenizer + the id-level loop
of nanollama_amd.engine.Engine."""
from __future__ import annotations

import codecs
import sys
from typing import Optional

from .engine import Engine, GenParams
from .model import LlamaModel
from .tokenizer import Tokenizer


OUTPUT_CAP = 8192   # bytes: the reference loop runs while len(output) < 8192 (go/main.go:173)


class TextOutput:
    """The text of one generation as its ids arrive: the pieces' bytes, the output cap and, when `stream` is given, an
    incremental UTF-8 decode written there piece by piece.  Shared by TextEngine and the batch scheduler."""

    def __init__(self, tokenizer: Tokenizer, stream=None):
        self.tokenizer, self.stream = tokenizer, stream
        self.out = bytearray()
        self.dec = codecs.getincrementaldecoder("utf-8")(errors="replace")

    def add(self, t: int) -> bool:
        """Append the piece of id t; True when the output reached the cap: the piece that crosses it is the last one
        emitted, and the caller samples no further token."""
        piece = self.tokenizer.decode_token_bytes(t)
        self.out.extend(piece)
        if self.stream is not None:
            self.stream.write(self.dec.decode(piece))
            self.stream.flush()
        return len(self.out) >= OUTPUT_CAP

    def finish_stream(self) -> None:
        """What the incremental decoder still holds, and the line end."""
        self.stream.write(self.dec.decode(b"", final=True) + "\n")

    def text(self) -> str:
        return bytes(self.out).decode("utf-8", errors="replace")


class TextEngine:
    def __init__(self, model: LlamaModel, tokenizer: Tokenizer, rep_penalty: float = 1.15, rep_window: int = 64,
                 seed: Optional[int] = None):
        self.model, self.tokenizer = model, tokenizer
        self.ids = Engine(model, eos_id=tokenizer.eos_id, rep_penalty=rep_penalty, rep_window=rep_window, seed=seed)

    def generate(self, prompt: str, p: GenParams, stream=None) -> str:
        """Generate (go/main.go:152): streams pieces to `stream` (stdout in the CLI), prints "[N tokens, X tok/s]"."""
        tokens = self.tokenizer.encode(prompt, True)
        out = TextOutput(self.tokenizer, stream)
        # on_token returning True (the cap) stops the id-level loop right there (no further sample)
        self.ids.generate_ids(tokens, p, on_token=out.add)
        if stream is not None:
            out.finish_stream()
            if self.ids.last_tokens and self.ids.last_tok_per_s > 0:
                stream.write("[%d tokens, %.1f tok/s]\n" % (self.ids.last_tokens, self.ids.last_tok_per_s))
            stream.flush()
        return out.text()

    def generate_quiet(self, prompt: str, p: GenParams) -> str:
        """GenerateQuiet (go/main.go:233-291)."""
        return self.generate(prompt, p, stream=None)
