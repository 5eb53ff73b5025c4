"""Learning agents that act on the batched environments."""
